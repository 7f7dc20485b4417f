"""Per-query label filters (Engine.set_labels / set_filters, bang_k_search_exact_labels: search_exact_labels_kernel and
search_exact_labels_pull_kernel of csrc/bang_search_exact.hip) on a GPU, against the CPU reference of tests/labels_reference.py: ids and distance
bits of the filtered answer, the matched counts, the four per-query counters, and -- the walk is untouched -- the candidate log of the same engine
run without filters.  32 queries per fixture; worklists of 10, 37 and 152 (k = 10, and k = L at L = 37); every table and batch of
tests/labels_inputs.py; graph entries in HBM and pulled rows.  Then int8, the toy inputs and the 65-id seed list in every layout, the mixed batch,
an exclusion set on top, one wave per workgroup, one allocation queried three times, device buffers, labels without filters, the refusals, the two
environment files and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
import exclude_reference as X
import labels_inputs as LI
import labels_reference as LR

pytestmark = pytest.mark.gpu

K = 10
NQ = 32
LS = (10, 37, 152)
FORMS = {"hbm": dict(graph=1, distance=1), "pull": dict(graph=0, pull=1, distance=1)}
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _traces(name, ix, q, L):
    return _cached((name, q.shape, L), lambda: LR.Reference(ix).walks(q, L))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(e, q, k, L, filters=None, Qcap=None):
    """A loaded, unallocated engine: one batch with the filters (any, all) or without.  -> (ids, dists, counters, log, counts, stats, matched)"""
    Q = q.shape[0]
    e.set_searchparams(k, L)
    e.alloc(Q if Qcap is None else Qcap)
    if filters is not None:
        e.set_filters(*filters)
    e.init(Q)
    ids, d = e.query(q)
    out = (ids, d, e.query_counters(Q)) + e.candidate_log(Q, L) + (e.stats(),)
    out += (e.matched_counts(Q) if filters is not None else None,)
    e.free()
    return out


def _check(got, want, base, what):
    """want = LR.collect_all(...); base = the same engine's run without filters"""
    ids, d, matched, st, _ = want
    assert np.array_equal(got[0], ids), what
    assert np.array_equal(_bits(got[1]), _bits(d)), what
    assert np.array_equal(got[6], matched), what
    assert np.array_equal(got[2], st), what
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[4], base[4]), what
    for i in range(len(got[4])):
        assert np.array_equal(got[3][i, :got[4][i]], base[3][i, :base[4][i]]), (what, i)


def _check_base(base, traces, k, what):
    for i, t in enumerate(traces):
        n = min(k, len(t.wl_ids))
        assert np.array_equal(base[0][i, :n], t.wl_ids[:n].astype(np.uint64)) and (base[0][i, n:] == LR.PAD_ID).all(), (what, i)
        assert np.array_equal(_bits(base[1][:n, i]), _bits(t.wl_dists[:n])), (what, i)
        assert tuple(base[2][i]) == tuple(t.stats), (what, i)
        assert np.array_equal(base[3][i, :base[4][i]], t.log), (what, i)


def _case(name, ix, q, opts, Ls, cases, ks=None, excluded=None):
    """cases: [(label, labels u32 [N], any, all)]"""
    import bang_amd
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        if excluded is not None:
            e.set_excluded(excluded)
        for L in Ls:
            tr = _traces(name, ix, q, L)
            base = None
            for label, labels, any_, all_ in cases(ix, np.array([t.wl_ids[0] for t in tr], np.uint64)):
                e.set_labels(labels)
                if base is None and excluded is None:
                    base = _run(e, q, K, L)                                     # labels loaded, no filters: today's launches
                    _check_base(base, tr, K, (name, L, "no filters"))
                    s = base[5]
                    assert s["label_launches"] == 0 and s["filtered_queries"] == 0 and s["labelled"] == ix.N and s["front_launches"] == 1, s
                elif base is None:
                    base = _run(e, q, K, L)
                for k in (ks(L) if ks else (K,)):
                    got = _run(e, q, k, L, (any_, all_))
                    want = LR.collect_all(tr, labels, any_, all_, k, L, int(ix.medoid), excluded)
                    _check(got, want, base, (name, L, label, k))
                    s = got[5]
                    assert s["label_launches"] == 1 and s["front_launches"] == 1 and s["exclude_launches"] == 0, s
                    assert s["filtered_queries"] == int(((any_ | all_) != 0).sum()), s
        e.unload()


def _named_cases(ix, rank0):
    Q = len(rank0)
    return [(f"{t}/{b}", LI.table(t, ix, rank0)) + LI.batch(b, Q) for t, b in LI.CASES]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_filtered_walks(request, fixture, form, L):
    ix, q, _, _ = request.getfixturevalue(fixture)
    _case(fixture, ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (L,), _named_cases, ks=lambda L_: (K, L_) if L_ == 37 else (K,))


@pytest.mark.parametrize("form", list(FORMS))
def test_int8(small_i8, form):
    ix, q, _, _ = small_i8
    _case("small_i8", ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (24,), _named_cases)


def _toy_cases(sets):
    """sets: lists of matching nodes; any = bit 0"""
    def make(ix, rank0):
        out = []
        for s in sets:
            labels = np.zeros(ix.N, np.uint32)
            labels[list(s(ix.N))] = 1
            out.append((str(len(list(s(ix.N)))), labels, np.ones(len(rank0), np.uint32), np.zeros(len(rank0), np.uint32)))
        return out
    return make


@pytest.mark.parametrize("form", list(FORMS))
def test_toy_inputs(form):
    """The chain with every third node (a full result list while the worklist holds three matches); row_dup with node 2 alone (in twice) and with
    everybody; the short worklist without node 1."""
    ix, q = E.chain()
    _case("chain", ix, q, FORMS[form], (10, 152), _toy_cases((lambda N: range(0, N, 3), lambda N: range(N), lambda N: [N - 1])))
    ix, q = BI.row_dup()
    _case("row_dup", ix, q, FORMS[form], (10,), _toy_cases((lambda N: [2], lambda N: range(N), lambda N: [4, 5])))
    ix, q = E.short_worklist()
    _case("short_worklist", ix, q, FORMS[form], (10,), _toy_cases((lambda N: [0, 2], lambda N: [1])))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed65(variant, dtype, D, form):
    """65 survivors in the seed iteration: 65 matches, 64 (one of the lanes' missing, the lane-less 65th missing), and the 65th alone."""
    ix, q = E.seed65(dtype, variant, D)
    sets = (lambda N: range(N), lambda N: [i for i in range(N) if i != 5], lambda N: range(64), lambda N: [64])
    _case(f"seed65-{dtype}-{variant}", ix, q, FORMS[form], (10,), _toy_cases(sets))


@pytest.mark.parametrize("form", list(FORMS))
def test_unfiltered_queries_of_a_mixed_batch_are_todays_answers(small_u8, form):
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    any_, all_ = LI.batch("mixed", NQ)
    with bang_amd.Engine(ix.dtype, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_labels(LI.rand4(ix.N))
        for L in LS:
            base = _run(e, q, K, L)
            got = _run(e, q, K, L, (any_, all_))
            assert np.array_equal(got[0][::3], base[0][::3]) and np.array_equal(_bits(got[1][:, ::3]), _bits(base[1][:, ::3])), L
            assert not np.array_equal(got[0], base[0])
        e.unload()


@pytest.mark.parametrize("form", list(FORMS))
def test_with_an_exclusion_set(small_u8, form):
    """A node of the engine's exclusion set never enters the result list; bang_k_worklist_pick is not launched for a filtered batch."""
    ix, q, _, _ = small_u8
    _case("small_u8", ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (37,), _named_cases, excluded=X.make_mask("rand30", ix))


@pytest.mark.parametrize("form", list(FORMS))
def test_one_wave_per_workgroup(small_u8, monkeypatch, form):
    """One workgroup of one wave runs every query in turn (the wave cap alone repeats the default launch: 32 queries are 32 one-wave workgroups
    already).  Full workgroups: tests/test_gpu_launch_shapes.py."""
    ix, q, _, _ = small_u8
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    _case("small_u8", ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (37,), _named_cases)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_allocation_three_queries(small_u8, form):
    """Filters set, replaced, cleared on one allocation: the last run is today's run."""
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    L = 37
    tr = _traces("small_u8", ix, q, L)
    labels = LI.rand4(ix.N)
    with bang_amd.Engine(ix.dtype, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_labels(labels)
        e.set_searchparams(K, L)
        e.alloc(NQ)
        for b in ("all2", "any_all"):
            any_, all_ = LI.batch(b, NQ)
            e.set_filters(any_, all_)
            e.init(NQ)
            ids, d = e.query(q)
            want = LR.collect_all(tr, labels, any_, all_, K, L, int(ix.medoid))
            assert np.array_equal(ids, want[0]) and np.array_equal(_bits(d), _bits(want[1])) and np.array_equal(e.matched_counts(NQ), want[2]), b
            assert e.stats()["label_launches"] == 1
        e.init(7)
        with pytest.raises(bang_amd.BangError, match="filters"):               # a batch of another size than the filters'
            e.query(q[:7])
        e.clear_filters()
        e.init(NQ)
        ids, d = e.query(q)
        _check_base((ids, d, e.query_counters(NQ)) + e.candidate_log(NQ, L), tr, K, "cleared")
        assert e.stats()["label_launches"] == 0 and e.stats()["filtered_queries"] == 0
        with pytest.raises(bang_amd.BangError, match="filters"):
            e.matched_counts(NQ)
        e.free()
        e.unload()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("with_dists", (True, False))
def test_results_into_device_buffers(small_u8, with_dists, form):
    import torch
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    L = 37
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("any_all", NQ)
    want = LR.collect_all(_traces("small_u8", ix, q, L), labels, any_, all_, K, L, int(ix.medoid))
    d_ids = torch.zeros((NQ, K), dtype=torch.int64, device="cuda")
    d_d = torch.zeros((K, NQ), dtype=torch.float32, device="cuda")
    with bang_amd.Engine(ix.dtype, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_labels(labels)
        e.set_searchparams(K, L)
        e.alloc(NQ)
        e.set_filters(any_, all_)
        e.init(NQ)
        e.query_dev(q, d_ids.data_ptr(), d_d.data_ptr() if with_dists else 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), want[0])
        if with_dists:
            assert np.array_equal(d_d.cpu().numpy().view(np.uint32), _bits(want[1]))
        else:
            assert not d_d.cpu().numpy().any()
        assert np.array_equal(e.matched_counts(NQ), want[2])
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# call order and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_call_order(small_u8):
    import bang_amd
    ix, q, _, _ = small_u8
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("all2", NQ)
    with bang_amd.Engine(ix.dtype, graph=1, distance=1) as e:
        with pytest.raises(bang_amd.BangError, match="no index is loaded"):
            e.set_labels(labels)
        e.load_index(ix)
        with pytest.raises(bang_amd.BangError, match=f"labels.*{ix.N - 1}.*{ix.N}"):
            e.set_labels(labels[:-1])
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):            # filters live in an allocation
            e.set_filters(any_, all_)
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        with pytest.raises(bang_amd.BangError, match="labels"):                # no labels set
            e.set_filters(any_, all_)
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):            # the rule of the options consumed by bang_alloc
            e.set_labels(labels)
        e.free()
        e.set_labels(labels)
        assert e.stats()["labelled"] == ix.N
        e.alloc(NQ)
        with pytest.raises(bang_amd.BangError, match="exceed"):
            e.set_filters(np.zeros(NQ + 1, np.uint32), np.zeros(NQ + 1, np.uint32))
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):
            e.clear_labels()
        e.free()
        e.clear_labels()
        assert e.stats()["labelled"] == 0
        e.set_labels(labels)
        e.unload()                                                             # drops the table
        e.load_index(ix)
        assert e.stats()["labelled"] == 0
        e.unload()


@pytest.mark.parametrize("opts,fixture", ((dict(graph=1), "small_u8"), (dict(graph=1, distance=1, beam=2), "small_u8"),
                                          (dict(graph=0, pull=1, distance=1, vectors_fp16=1), "small_f32"), (dict(graph=1, distance=1), "u8_48")),
                         ids=("pq_walk", "beam", "fp16", "wide"))
def test_forms_without_a_label_filter_kernel_are_refused(request, opts, fixture):
    """Refused at set_filters with `labels` in the message; the same engine runs its unfiltered batch."""
    import bang_amd
    if fixture == "u8_48":
        import highdim_inputs as H
        ix, q = H.get("u8_48")
    else:
        ix, q, _, _ = request.getfixturevalue(fixture)
    q = np.ascontiguousarray(q[:8])
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        e.set_labels(np.ones(ix.N, np.uint32))
        e.set_searchparams(K, 24)
        e.alloc(8)
        with pytest.raises(bang_amd.BangError, match="labels"):
            e.set_filters(np.ones(8, np.uint32), np.zeros(8, np.uint32))
        e.init(8)
        ids, _ = e.query(q)
        assert (ids != LR.PAD_ID).any() and e.stats()["label_launches"] == 0
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the environment files: bang.h callers and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _entry_source(ix):
    """A Python entry source over an in-memory index (bang_load_stream_e): copies the requested node range in the reference entry layout."""
    import ctypes as C
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)

    def src(first, count, dst):
        C.memmove(dst, graph[first:first + count].ctypes.data, count * ix.entry_len)
        return 0
    return src


LOADS = ("mem", "file", "stream", "shared")                 # bang_load_mem_e, bang_load_e, bang_load_stream_e, bang_load_shared_e


@pytest.mark.parametrize("load", LOADS)
def test_label_file_is_read_by_every_load(small_i8, tmp_path, monkeypatch, load):
    """BANG_LABEL_FILE through each of the four loads: a filtered batch on the loaded engine equals the reference; a bad file -- too few labels, missing,
    another layout -- fails that load with the variable, the file and the reason named, and leaves nothing behind: the same engine then loads without
    the variable and carries no labels."""
    import bang_amd
    from bang_amd import binding as B
    from bang_amd import formats
    ix, q, _, _ = small_i8
    q = np.ascontiguousarray(q[:NQ])
    L = 24
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("any_all", NQ)
    good = str(tmp_path / "labels.bin")
    formats.write_bin(good, labels.reshape(-1, 1))
    short = str(tmp_path / "short.bin")
    formats.write_bin(short, labels[:-1].reshape(-1, 1))
    odd = str(tmp_path / "odd.bin")
    with open(odd, "wb") as f:                                             # two columns, and a byte too many
        f.write(np.array([3, 2], np.int32).tobytes() + bytes(25))
    huge = str(tmp_path / "huge.bin")
    with open(huge, "wb") as f:                                            # a header that promises 2^31 - 1 words in a file of 16 bytes
        f.write(np.array([0x7FFFFFFF, 1], np.int32).tobytes() + bytes(8))
    bad = ((short, "labels"), (str(tmp_path / "missing.bin"), "cannot be opened"), (odd, "not a .bin file"), (huge, "not a .bin file"))
    want = LR.collect_all(_traces("small_i8", ix, q, L), labels, any_, all_, K, L, int(ix.medoid))
    monkeypatch.setenv("BANG_PULL_ROWS_DIR", str(tmp_path))
    prefix = str(tmp_path / "ix")
    opts = dict(graph=1, distance=1) if load == "mem" else dict(graph=0, pull=1, distance=1)
    bufs = []
    sibling = None
    if load == "file":
        formats.write_index(prefix, ix)
    if load == "shared":                                                   # the node's loading rank: its vectors and its rows file
        v1, v2 = B.DeviceBuffer(ix.N * ix.D + 256), B.DeviceBuffer(ix.N * ix.D + 256)
        bufs = [v1, v2]
        sibling = bang_amd.Engine(ix.dtype, graph=0)
        sibling.load_stream(ix, _entry_source(ix), d_vectors=v1.ptr)
        rows_hash = sibling.rows_hash()
        v2.upload(v1.download(np.uint8, (ix.N * ix.D,)))

    def do_load(e):
        if load == "mem":
            e.load_index(ix)
        elif load == "file":
            e.load(prefix)
        elif load == "stream":
            e.load_stream(ix, _entry_source(ix))
        else:
            e.load_shared(ix, bufs[1].ptr, rows_hash)
    try:
        monkeypatch.setenv("BANG_LABEL_FILE", good)
        with bang_amd.Engine(ix.dtype, **opts) as e:
            do_load(e)
            got = _run(e, q, K, L, (any_, all_))
            assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[6], want[2])
            assert got[5]["labelled"] == ix.N and got[5]["label_launches"] == 1
            e.unload()
        for p, word in bad:
            monkeypatch.setenv("BANG_LABEL_FILE", p)
            with bang_amd.Engine(ix.dtype, **opts) as e:
                with pytest.raises(bang_amd.BangError) as err:
                    do_load(e)
                assert word in str(err.value) and p in str(err.value) and "BANG_LABEL_FILE" in str(err.value), str(err.value)
                monkeypatch.delenv("BANG_LABEL_FILE")
                do_load(e)                                                 # (the failed load left nothing behind)
                assert e.stats()["labelled"] == 0
                e.unload()
    finally:
        if sibling is not None:
            sibling.close()
        for b in bufs:
            b.free()


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_LABEL_FILE + BANG_QUERY_FILTER_FILE, BANG_DISTANCE=exact BANG_GRAPH=device bang_search (interactive L): the recall it prints at each L
    is that of the reference's ids, and differs from the unfiltered one.  A filter file with fewer rows than queries ends the run."""
    import bang_amd
    from bang_amd import formats
    from oracle import oracle as O
    ix, q, gt_i, gt_d = small_i8
    Q = q.shape[0]
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("mixed", Q)
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    formats.write_truthset(str(tmp_path / "gt.bin"), gt_i, gt_d)
    formats.write_bin(str(tmp_path / "labels.bin"), labels.reshape(-1, 1))
    formats.write_bin(str(tmp_path / "f.bin"), np.stack([any_, all_], axis=1))
    formats.write_bin(str(tmp_path / "few.bin"), np.stack([any_, all_], axis=1)[:Q - 1])
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    Ls = (10, 37)
    env = dict(os.environ, BANG_LABEL_FILE=str(tmp_path / "labels.bin"), BANG_QUERY_FILTER_FILE=str(tmp_path / "f.bin"), BANG_GRAPH="device",
               BANG_DISTANCE="exact")
    args = [exe, prefix, str(tmp_path / "q.bin"), str(tmp_path / "gt.bin"), str(Q), "10", "int8", "l2"]
    out = subprocess.run(args, input="".join(f"{L}\ny\n" for L in Ls[:-1]) + f"{Ls[-1]}\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split("\t") for l in out.stdout.splitlines() if l[:1].isdigit() and l.count("\t") == 3]
    assert "10-r@10" in out.stdout and sorted({int(r[0]) for r in rows}) == list(Ls)
    for L in Ls:
        tr = _traces("small_i8_all", ix, q, L)
        ids = LR.collect_all(tr, labels, any_, all_, K, L, int(ix.medoid))[0]
        zero = np.zeros(Q, np.uint32)
        ids_u = LR.collect_all(tr, labels, zero, zero, K, L, int(ix.medoid))[0]
        unfiltered = f"{float(np.float32(O.recall(gt_i, gt_d, ids_u, 10))):.2f}"
        want = f"{float(np.float32(O.recall(gt_i, gt_d, ids, 10))):.2f}"
        got = [r_[3].strip() for r_ in rows if int(r_[0]) == L]
        assert want != unfiltered                                          # (a run that ignored the files would print this)
        assert len(got) == 5 and all(g == want for g in got), (L, got, want)
    env["BANG_QUERY_FILTER_FILE"] = str(tmp_path / "few.bin")
    out = subprocess.run(args, input="10\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "BANG_QUERY_FILTER_FILE" in out.stderr and "filters" in out.stderr, out.stderr[-2000:]
