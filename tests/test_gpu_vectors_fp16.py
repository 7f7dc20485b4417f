"""Option vectors_fp16 on the GPU: a float index on the host placement keeps its HBM vector table as IEEE fp16 (converted on the GPU at load,
csrc/bang_kernels.hip f32_to_f16_kernel), the re-rank launch (rerank_f16_kernel) and the exact-distance kernel's pulled-rows form
(search_exact_pull_f16_kernel) read it.  fp16 -> fp32 is exact, so every run equals the CPU reference on the index with its vectors rounded
(tests/fp16_inputs.py) bit for bit: ids, distance bits and the four per-query counters.  tests/test_fp16_inputs.py asserts that this reference
differs from the one on the original index for every input used here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import base_forms as F
import edge_inputs as E
import fp16_inputs as H

pytestmark = pytest.mark.gpu

# the three host-placement forms whose re-rank reads the vector table
FORMS = {"pull": dict(pull=1), "walker": dict(pull=1, walker=1), "loop": dict(persistent=0, vectors=1)}
RERANK_INPUTS = ("small_f32", "small_deep", "synth7", "synth33", "synth100", "synth260")
LS = (10, 37, 152)


def _input(name, request):
    if name.startswith("synth"):
        return H.synth_index(int(name[5:]))
    return request.getfixturevalue(name)[:2]


def _engine(ix, fp16=1, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, vectors_fp16=fp16, **opts)
    try:
        e.load_index(ix)
    except BaseException:
        e.close()
        raise
    return e


def _run(e, q, k, L, distfn=0, Q=None):
    e.set_searchparams(k, L, distfn)
    e.alloc(q.shape[0] if Q is None else Q)
    e.init(q.shape[0])
    ids, d = e.query(q)
    return ids, d, e.query_counters(q.shape[0])


def _assert_same(e, got, want):
    ids, d, st = got
    ids_r, d_r, st_r = want
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
    if e.stats()["search_kernel"]:
        assert np.array_equal(st, st_r)                       # iterations, candidates, dist_evals, fetched
    else:
        assert np.array_equal(st[:, 1:], st_r[:, 1:])         # (the launch-per-iteration loop reports no per-query iterations)


def _assert_fp16_stats(e, ix):
    s = e.stats()
    assert s["vectors_fp16"] == 1 and s["vector_table_bytes"] == H.table_bytes(ix.N, ix.D), s
    assert s["vectors_on_device"] == 1 and s["rerank_fused"] == 0 and s["graph_mode"] == 0, s
    return s


# ------------------------------------------------------------------------------------------------------------------------ conversion kernel
def _convert(src: np.ndarray, src_stride: int, dst_stride: int):
    """bang_k_f32_to_f16 alone: src [rows][D] f32 laid out at src_stride bytes -> (halves [rows][D] as u16, padding bytes, bad count)."""
    from bang_amd import binding as B
    rows, D = src.shape
    host = np.zeros((rows, src_stride // 4), np.float32)
    host[:, :D] = src
    d_src = B.DeviceBuffer.from_numpy(host)
    d_dst = B.DeviceBuffer(rows * dst_stride + 256)
    B._check(B.lib().bang_dev_memset(C.c_void_p(d_dst.ptr), 0xAB, C.c_size_t(d_dst.nbytes)), "memset")
    d_bad = B.DeviceBuffer(4)
    fn = B.lib().bang_k_f32_to_f16
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    B._check(fn(d_src.ptr, d_dst.ptr, rows, D, src_stride, dst_stride, d_bad.ptr, None), "bang_k_f32_to_f16")
    B.sync()
    raw = d_dst.download(np.uint8, (rows * dst_stride + 256,))
    bad = int(d_bad.download(np.uint32, (1,))[0])
    for b in (d_src, d_dst, d_bad):
        b.free()
    body = raw[:rows * dst_stride].reshape(rows, dst_stride)
    halves = body[:, :2 * D].copy().view(np.uint16).reshape(rows, D)
    return halves, body[:, 2 * D:], raw[rows * dst_stride:], bad


@pytest.mark.parametrize("D", [1, 7, 96, 260])
def test_conversion_kernel_matches_numpy(D):
    """Round to nearest even, subnormals produced, +-0, the largest half, strides unequal to the row; the padding half of an odd row is 0 and
    nothing outside the rows is written."""
    rng = np.random.default_rng(D)
    rows = 37
    special = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14,
                        2.0 ** -14 * (1 - 2.0 ** -12), 0.0, -0.0, 65504.0, -65504.0, 65519.99, -65519.99, 6e-8, 6e-5, 1e-6, 3.3e-6, 1e-40, np.inf, -np.inf],
                       np.float32)
    src = np.concatenate([rng.standard_normal(rows * D * 2 // 4 + 8).astype(np.float32) * 100.0,
                          np.exp(rng.uniform(np.log(6e-8), np.log(6e-5), rows * D)).astype(np.float32) * rng.choice([-1.0, 1.0], rows * D).astype(np.float32),
                          np.tile(special, 1 + rows * D // special.size)])
    src = np.ascontiguousarray(rng.permutation(src)[:rows * D].reshape(rows, D))
    src.flat[:min(special.size, src.size)] = special[:min(special.size, src.size)]
    row = H.row_bytes(D)
    with np.errstate(over="ignore"):
        want = src.astype(np.float16).view(np.uint16)
    for src_stride, dst_stride in ((4 * D, row), (4 * D + 12, row + 8)):
        got, pad, slack, bad = _convert(src, src_stride, dst_stride)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        assert bad == 0
        assert np.all(pad[:, :row - 2 * D] == 0) and np.all(pad[:, row - 2 * D:] == 0xAB)      # the padding half; nothing behind the row
        assert np.all(slack == 0xAB)


def test_conversion_kernel_counts_what_leaves_the_range():
    """65520 is the first float that rounds to inf: it is converted (inf) AND counted; 65519.99 rounds to 65504 and is not; NaN stays NaN."""
    src = np.zeros((5, 8), np.float32)
    src[0, 0], src[0, 1], src[1, 7], src[2, 3], src[4, 4], src[4, 5] = 65520.0, 65519.99, -65520.0, 1e5, np.nan, np.inf
    src[3, :] = 3.4e38
    got, _, _, bad = _convert(src, 32, 16)
    assert bad == 3 + 8
    with np.errstate(over="ignore"):
        want = src.astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want)
    assert got[0, 0] == 0x7C00 and got[0, 1] == 0x7BFF and got[1, 7] == 0xFC00 and (got[4, 4] & 0x7C00) == 0x7C00 and (got[4, 4] & 0x3FF) != 0


# ------------------------------------------------------------------------------------------------------------------------ re-rank
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", RERANK_INPUTS)
def test_rerank_reads_the_rounded_vectors(name, form, request):
    """Every host-placement form whose re-rank reads the table; D = 7 (a padding half), 33, 100 (D % 8 != 0), 260 (a second fetch tile)."""
    import bang_amd
    ix, q = _input(name, request)
    rix = H.rounded(ix)
    with _engine(ix, **FORMS[form]) as e:
        if name == "synth260" and form == "walker":
            # a layout on the LUT path has no search-kernel instance: the host-paced form is refused -- with the option and, the same
            # refusal, without it (a limitation the option found, not one it made)
            for eng in (e, _engine(ix, fp16=0, **FORMS[form])):
                eng.set_searchparams(10, 37)
                with pytest.raises(bang_amd.BangError, match="option walker = 1: the host-paced search kernel is not available"):
                    eng.alloc(q.shape[0])
                if eng is not e:
                    eng.close()
            return
        for L in LS:
            for k in (1, 10, L):
                _assert_same(e, _run(e, q, k, L), H.pq_reference((name, "r"), rix, q, k, L))
                s = _assert_fp16_stats(e, ix)
                if form == "loop" or name == "synth260":
                    assert s["search_kernel"] == 0 and s["persistent"] == 0, s
                elif form == "pull":
                    assert s["graph_pull"] == 1 and s["search_kernel"] == 1 and s["walker_threads"] == 0, s
                else:
                    assert s["search_kernel"] == 1 and s["walker_rows"] == 1 and s["pacing_groups"] > 0, s
                e.free()


@pytest.mark.parametrize("form", ["pull", "loop"])
def test_mips(small_f32, form):
    import bang_amd
    ix, q = small_f32[:2]
    q1 = np.ascontiguousarray(q[:, :-1])
    with _engine(ix, **FORMS[form]) as e:
        _assert_same(e, _run(e, q1, 10, 37, bang_amd.DIST_MIPS), H.pq_reference(("small_f32", "r"), H.rounded(ix), q1, 10, 37, mips=True))
        _assert_fp16_stats(e, ix)
        e.free()


def test_batch_sizes(small_deep):
    ix, q = small_deep[:2]
    k, L = 10, 37
    qq = np.ascontiguousarray(np.tile(q, (18, 1))[:700])
    want = H.pq_reference(("small_deep", "r700"), H.rounded(ix), qq, k, L)
    with _engine(ix, pull=1) as e:
        for Q in (1, 700):
            _assert_same(e, _run(e, qq[:Q], k, L), (want[0][:Q], np.ascontiguousarray(want[1][:, :Q]), want[2][:Q]))
            _assert_fp16_stats(e, ix)
            e.free()


@pytest.mark.parametrize("form", ["pull", "loop"])
def test_ties_created_by_rounding(small_f32, form):
    """Pairs of nodes that differ only below fp16 precision are ONE vector in the table: exact ties, ranked by expansion order."""
    ix, q = H.rounding_ties(*small_f32[:2])
    want = H.pq_reference(("ties", "r"), H.rounded(ix), q, 10, 37)
    assert E.ties_in_top(want[1], 10).any()
    with _engine(ix, **FORMS[form]) as e:
        _assert_same(e, _run(e, q, 10, 37), want)
        e.free()


# ------------------------------------------------------------------------------------------------------------------------ ways in
def _entry_source(ix):
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)

    def src(first, count, dst):
        C.memmove(dst, graph[first:first + count].ctypes.data, count * ix.entry_len)
        return 0
    return src


@pytest.mark.timeout(300, method="thread")
def test_every_way_in_builds_the_same_table(small_deep, tmp_path):
    """load_index (resident graph: the copy loop), load_stream with an entry source and index files through Engine.load (streamed)."""
    import bang_amd
    from bang_amd import formats
    ix, q = small_deep[:2]
    k, L = 10, 37
    want = H.pq_reference(("small_deep", "r"), H.rounded(ix), q, k, L)
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    loaders = (lambda e: e.load_index(ix), lambda e: e.load_stream(ix, _entry_source(ix)), lambda e: e.load(prefix))
    for load in loaders:
        with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, vectors_fp16=1) as e:
            load(e)
            _assert_same(e, _run(e, q, k, L), want)
            s = _assert_fp16_stats(e, ix)
            assert s["graph_pull"] == 1, s
            e.free()
            e.unload()


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_deep, tmp_path):
    """BANG_VECTORS_FP16=1 BANG_GRAPH=host bang_search prints the usual table; its recall at each L is that of the reference on the rounded index."""
    import bang_amd
    from bang_amd import formats
    from oracle import oracle as O
    ix, q, gt_i, gt_d = small_deep
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    formats.write_truthset(str(tmp_path / "gt.bin"), gt_i, gt_d)
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    Ls = (10, 37)
    env = dict(os.environ, BANG_VECTORS_FP16="1", BANG_GRAPH="host")
    out = subprocess.run([exe, prefix, str(tmp_path / "q.bin"), str(tmp_path / "gt.bin"), str(q.shape[0]), "10", "float", "l2"],
                         input="".join(f"{L}\ny\n" for L in Ls[:-1]) + f"{Ls[-1]}\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split("\t") for l in out.stdout.splitlines() if l[:1].isdigit() and l.count("\t") == 3]
    assert "10-r@10" in out.stdout and sorted({int(r[0]) for r in rows}) == list(Ls)
    for L in Ls:
        ids, _, _ = H.pq_reference(("small_deep", "r"), H.rounded(ix), q, 10, L)
        want = f"{float(np.float32(O.recall(gt_i, gt_d, ids, 10))):.2f}"
        got = [r[3].strip() for r in rows if int(r[0]) == L]
        assert len(got) == 5 and all(g == want for g in got), (L, got, want)


# ------------------------------------------------------------------------------------------------------------------------ exact mode
def _exact_engine(ix, **opts):
    import bang_amd
    return _engine(ix, pull=1, distance=bang_amd.DISTANCE_EXACT, **opts)


def _assert_exact_stats(e, ix):
    s = _assert_fp16_stats(e, ix)
    assert s["graph_pull"] == 1 and s["search_kernel"] == 1 and s["front_launches"] == 1 and s["walker_threads"] == 0, s
    return s


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", ["small_deep", "synth256"])
def test_exact_mode_on_fp16_rows(name, request):
    ix, q = _input(name, request)
    rix = H.rounded(ix)
    Q = q.shape[0]
    with _exact_engine(ix) as e:
        for L in LS:
            _assert_same(e, _run(e, q, 10, L), H.exact_reference((name, "r"), rix, q, 10, L))
            s = _assert_exact_stats(e, ix)
            assert s["rows_in_hbm"] == 0 and s["pulled_bytes"] == 256 * (int(s["candidates"]) - Q), s
            e.free()


@pytest.mark.timeout(300, method="thread")
def test_exact_mode_with_the_rows_in_hbm(small_deep):
    """rows_hbm forced to 0 and to all rows: the row source does not change a bit."""
    ix, q = small_deep[:2]
    want = H.exact_reference(("small_deep", "r"), H.rounded(ix), q, 10, 37)
    for rows_hbm, n_hbm in ((0, 0), (64, ix.N)):
        with _exact_engine(ix, rows_hbm=rows_hbm) as e:
            _assert_same(e, _run(e, q, 10, 37), want)
            s = _assert_exact_stats(e, ix)
            assert s["rows_in_hbm"] == n_hbm and (s["pulled_bytes"] == 0) == (n_hbm != 0), s
            e.free()
            e.unload()


@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_exact_mode_seed_list_of_65(variant):
    toy, q = E.seed65("float", variant, 128)
    ix = H.off_grid(toy)
    with _exact_engine(ix) as e:
        for L in (4, 10, 37):
            _assert_same(e, _run(e, q, 4, L), H.exact_reference(("seed65", variant, "r"), H.rounded(ix), q, 4, L))
            _assert_exact_stats(e, ix)
            e.free()


def test_exact_mode_chain_runs_to_the_cap():
    toy, q = E.chain("float", 128)
    ix = H.off_grid(toy)
    with _exact_engine(ix) as e:
        for L in (10, 37):
            cap = L + 49
            ref = H.exact_reference(("chain", "r"), H.rounded(ix), q, 10, L)
            assert ref[2][0].tolist() == [cap, cap + 1, cap + 1, cap + 1]
            _assert_same(e, _run(e, q, 10, L), ref)
            e.free()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_at_load(small_u8, small_deep):
    import bang_amd
    from bang_amd import binding as B
    ix8 = small_u8[0]
    ix = small_deep[0]
    with bang_amd.Engine("uint8", graph=0, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.*8-bit"):
            e.load_index(ix8)
    with bang_amd.Engine("float", graph=bang_amd.GRAPH_DEVICE, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.*graph = device"):
            e.load_index(ix)
    with bang_amd.Engine("float", graph=0, vectors=0, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.*vectors = 0"):
            e.load_index(ix)
    buf = B.DeviceBuffer(ix.N * ix.D * 4 + 256)
    with bang_amd.Engine("float", graph=0, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.*shared load"):
            e.load_shared(ix, buf.ptr, 0)
    with bang_amd.Engine("float", graph=0, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.*d_vectors"):
            e.load_stream(ix, _entry_source(ix), d_vectors=buf.ptr)
    buf.free()


def test_a_value_beyond_the_fp16_range_fails_the_load(small_deep):
    """Nothing is silently turned into inf: the load fails and the message carries the count; the same index loads without the option."""
    import dataclasses
    import bang_amd
    from bang_amd.formats import pack_graph
    ix, q = small_deep[:2]
    v = ix.vectors()
    v[5, 3], v[77, 0], v[ix.N - 1, ix.D - 1] = 1e5, -1e5, 65520.0
    bad = dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency()))
    for load in (lambda e: e.load_index(bad), lambda e: e.load_stream(bad, _entry_source(bad))):
        with bang_amd.Engine("float", graph=0, vectors_fp16=1) as e:
            with pytest.raises(bang_amd.BangError, match=r"code -5.*vectors_fp16.* 3 vector elements"):
                load(e)
    with bang_amd.Engine("float", graph=0) as e:
        e.load_index(bad)


@pytest.mark.parametrize("D", [100, 260])
def test_exact_mode_refuses_the_wide_layouts(D):
    import bang_amd
    ix, q = H.synth_index(D)
    with _exact_engine(ix) as e:
        e.set_searchparams(10, 37)
        with pytest.raises(bang_amd.BangError, match=r"code -5.*distance = 1.*vectors_fp16"):
            e.alloc(q.shape[0])


# ------------------------------------------------------------------------------------------------------------------------ default untouched
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", RERANK_INPUTS)
def test_default_is_untouched(name, form, request):
    """vectors_fp16 = 0 on every input and form of the re-rank test: the reference on the ORIGINAL index, a float table, the re-rank fused where it
    was (the pulled self-paced form on a layout bang_search_can_rerank accepts)."""
    if name == "synth260" and form == "walker":
        return                                                    # (refused with or without the option: test_rerank_reads_the_rounded_vectors)
    ix, q = _input(name, request)
    with _engine(ix, fp16=0, **FORMS[form]) as e:
        _assert_same(e, _run(e, q, 10, 37), H.pq_reference((name, "o"), ix, q, 10, 37))
        s = e.stats()
        assert s["vectors_fp16"] == 0 and s["vector_table_bytes"] == ix.N * ix.D * 4 + 256 and s["vectors_on_device"] == 1, s
        assert s["rerank_fused"] == int(form == "pull" and name != "synth260" and F.fusable(ix.dtype, ix.D, ix.D * 4)), s
        e.free()


def test_default_exact_mode_is_untouched(small_deep):
    ix, q = small_deep[:2]
    import bang_amd
    with _engine(ix, fp16=0, pull=1, distance=bang_amd.DISTANCE_EXACT) as e:
        _assert_same(e, _run(e, q, 10, 37), H.exact_reference(("small_deep", "o"), ix, q, 10, 37))
        assert e.stats()["vectors_fp16"] == 0
        e.free()
