"""The exact scan on the GPU (bang_scan_e, bang_k_scan; DESIGN.md section 2 CANON 23): ids, distance bits and matched counts compared bit for bit with
the CPU reference (tests/scan_reference.py: orc_exact_dist of all N points, masks in numpy, np.sort of the keys) for every query of every input of
tests/scan_inputs.py."""
import ctypes as C

import numpy as np
import pytest

import consolidate_inputs as CI
import insert_inputs as I
import scan_inputs as SI
import scan_reference as SR
import stretch_inputs as ST

pytestmark = pytest.mark.gpu

INPUTS = SI.FIXTURES + tuple(sorted(SI.SMALL)) + ("extremes_uint8", "extremes_int8", "ties_u8", "ties_f32")


def _input(request, name):
    """-> (Index, queries)"""
    if name in SI.FIXTURES:
        return request.getfixturevalue(name)[:2]
    if name in SI.SMALL:
        return SI.small(name)
    if name.startswith("extremes_"):
        return SI.extremes(name[9:])
    return SI.ties(name[5:])[:2]


def _engine(ix, **opts):
    import bang_amd
    opts.setdefault("graph", bang_amd.GRAPH_DEVICE)
    e = bang_amd.Engine(ix.dtype, **opts)
    e.load_index(ix)
    return e


def _same(got, want, what):
    assert SR.same(got, want), (what, SR.first_difference(got, want))


@pytest.mark.parametrize("name", INPUTS)
def test_every_input_at_every_k(request, name):
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    with _engine(ix) as e:
        for k in SI.KS:
            _same(e.scan(q, k), SR.answer(d, k), (name, k))
        t = e.scan_times()
        assert t["total"] > 0 and t["scan"] > 0 and t["merge"] > 0


@pytest.mark.parametrize("excl", SI.EXCLUSIONS)
@pytest.mark.parametrize("name", SI.FIXTURES)
def test_exclusion_sets(request, name, excl):
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    x = SI.exclusion(excl, d)
    with _engine(ix) as e:
        e.set_excluded(x)
        for k in SI.KS:                                                    # all_but: three candidates, k = 10, 100, 128 greater than that
            _same(e.scan(q, k), SR.answer(d, k, excluded=x), (name, excl, k))


@pytest.mark.parametrize("table,batch", SI.LABEL_CASES)
@pytest.mark.parametrize("name", SI.FIXTURES)
def test_label_filters(request, name, table, batch):
    ix, q = _input(request, name)
    Q = min(q.shape[0], 32) if table == "one_node" else q.shape[0]         # (one_node gives each query a label bit of its own: 32 at the most)
    d = SR.distances(ix, q)[:Q]
    q = np.ascontiguousarray(q[:Q])
    lab, a, b = SI.label_case(table, batch, ix, Q, d)
    x = SI.excl_edges(ix.N)
    with _engine(ix) as e:
        e.set_labels(lab)
        for k in SI.KS:
            _same(e.scan(q, k, a, b), SR.answer(d, k, labels=lab, any_=a, all_=b), (name, table, batch, k))
        _same(e.scan(q, 10), SR.answer(d, 10), (name, table, "no filters with a label table"))
        e.set_excluded(x)                                                  # filter and exclusion set together
        for k in SI.KS:
            _same(e.scan(q, k, a, b), SR.answer(d, k, excluded=x, labels=lab, any_=a, all_=b), (name, table, batch, "excluded", k))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel-level entry
# ---------------------------------------------------------------------------------------------------------------------
def _k_scan(ix, d_vec, stride, q, n_nodes, k, stripes=0, excluded=None, removed=None, labels=None, filters=None):
    from bang_amd import binding as B
    lib = B.lib()
    lib.bang_scan_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.bang_scan_scratch_bytes.restype = C.c_uint64
    lib.bang_scan_max_stripes.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    lib.bang_scan_max_stripes.restype = C.c_uint32
    Q = q.shape[0]
    most = lib.bang_scan_max_stripes(B.DTYPE_CODE[ix.dtype], n_nodes, k)
    nbytes = int(lib.bang_scan_scratch_bytes(Q, k, max(most, 1)))
    bufs = dict(q=B.DeviceBuffer.from_numpy(np.ascontiguousarray(q)), scratch=B.DeviceBuffer(nbytes), ids=B.DeviceBuffer(Q * k * 8),
                dists=B.DeviceBuffer(Q * k * 4), matched=B.DeviceBuffer(Q * 4))
    words = (ix.N + 31) // 32 + 1
    for key, ids in (("excluded", excluded), ("removed", removed)):
        if ids is not None:
            bits = np.zeros(words, np.uint32)
            np.bitwise_or.at(bits, np.asarray(ids, np.int64) >> 5, np.uint32(1) << (np.asarray(ids, np.uint32) & np.uint32(31)))
            bufs[key] = B.DeviceBuffer.from_numpy(bits)
    if labels is not None:
        bufs["labels"] = B.DeviceBuffer.from_numpy(np.ascontiguousarray(labels, np.uint32))
        bufs["filters"] = B.DeviceBuffer.from_numpy(np.ascontiguousarray(np.stack(filters, axis=1), np.uint32))
    p = B.ScanParams()
    p.d_vec_base, p.vec_stride, p.dtype, p.D, p.n_nodes = d_vec, stride, B.DTYPE_CODE[ix.dtype], ix.D, n_nodes
    p.d_queries, p.nq, p.k, p.stripes = bufs["q"].ptr, Q, k, stripes
    for key in ("excluded", "removed", "labels", "filters"):
        setattr(p, "d_" + key, bufs[key].ptr if key in bufs else None)
    p.d_scratch, p.scratch_bytes = bufs["scratch"].ptr, nbytes
    p.d_ids_out, p.d_dists_out, p.d_matched = bufs["ids"].ptr, bufs["dists"].ptr, bufs["matched"].ptr
    lib.bang_k_scan.argtypes = [C.c_void_p, C.c_void_p]
    rc = lib.bang_k_scan(C.byref(p), None)
    assert rc == 0, lib.bang_last_error().decode()
    B.sync()
    out = (bufs["ids"].download(np.uint64, (Q, k)), bufs["dists"].download(np.float32, (k, Q)), bufs["matched"].download(np.uint32, (Q,)))
    for b in bufs.values():
        b.free()
    return out, most


@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_kernel_entry_on_prefixes(request, name):
    """n_nodes = 1, 31, 32, 33, 63, 64, 65 and N at k = 100: more results asked for than there are candidates, tiles that end inside a wave"""
    from bang_amd import binding as B
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    graph = B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.graph), slack=256)
    try:
        for n in SI.N_PREFIXES + (ix.N,):
            got, _ = _k_scan(ix, graph.ptr, ix.entry_len, q, n, 100)
            _same(got, SR.answer(d, 100, n_nodes=n), (name, n))
        x, r = SI.excl_edges(ix.N), np.array([1, 33, 64, ix.N - 2], np.uint32)      # both bitmaps and a filter batch at the entry itself
        lab, a, b = SI.label_case("rand4", "mixed", ix, q.shape[0], d)
        got, _ = _k_scan(ix, graph.ptr, ix.entry_len, q, ix.N, 10, excluded=x, removed=r, labels=lab, filters=(a, b))
        _same(got, SR.answer(d, 10, excluded=x, removed=r, labels=lab, any_=a, all_=b), (name, "bitmaps + filters"))
    finally:
        graph.free()


@pytest.mark.parametrize("name", ["small_u8", "small_f32", "ties_u8", "ties_f32"])
def test_stripes_at_the_kernel_entry(request, name):
    """stripes = 1, 2, 7 and the largest a launch accepts: identical answers"""
    from bang_amd import binding as B
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    graph = B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.graph), slack=256)
    try:
        for k in (10, 128):
            want = SR.answer(d, k)
            _, most = _k_scan(ix, graph.ptr, ix.entry_len, q, ix.N, k, 1)
            assert most >= 1
            for s in sorted({1, min(2, most), min(7, most), most}):
                got, _ = _k_scan(ix, graph.ptr, ix.entry_len, q, ix.N, k, s)
                _same(got, want, (name, k, s))
    finally:
        graph.free()


@pytest.mark.parametrize("name", ["u8_128_m70", "i8_64_m16", "f32_128_m32"])
def test_stretched_stride(name):
    """rows 32 MiB apart: ids >= 128 lie beyond 4 GiB, ids >= 512 beyond 16 GiB; the expected answer is the compact index's"""
    ix, q = ST.get(name)
    d = SR.distances(ix, q)
    stride = ST.stride_of(ix.entry_len)
    assert 128 * stride > (4 << 30) and 512 * stride > (16 << 30) and ix.N > 512
    buf, ptr = ST.stretched(ix.graph, stride)
    try:
        for stripes in (1, 3):
            got, _ = _k_scan(ix, ptr, stride, q, ix.N, ST.K, stripes)
            want = SR.answer(d, ST.K)
            _same(got, want, (name, stripes))
        assert (want[0] >= 512).any() and (want[0] >= 128).any(), "no answer lies beyond the marks: the case would show nothing"
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", SI.QS)
@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_query_counts(request, name, Q):
    """1, 31, 33 and 130 queries: the seams of the query tiles (32 / 16) and a workgroup column's later tiles"""
    ix, q = _input(request, name)
    d = SI.tile_dist(SR.distances(ix, q), Q)
    qq = SI.queries_of(q, Q)
    with _engine(ix) as e:
        _same(e.scan(qq, 10), SR.answer(d, 10), (name, Q))


@pytest.mark.parametrize("name", ["small_u8", "small_deep", "ties_u8", "ties_f32"])
def test_the_hooks_change_nothing(request, name, monkeypatch):
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    want = {k: SR.answer(d, k) for k in (10, 128)}
    with _engine(ix) as e:
        for stripes in ("1", "2", "7", "100000", "0"):                     # 100000: clamped to the largest allowed; 0: the default
            monkeypatch.setenv("BANG_SCAN_STRIPES", stripes)
            for k in (10, 128):
                _same(e.scan(q, k), want[k], (name, "stripes", stripes, k))
        monkeypatch.delenv("BANG_SCAN_STRIPES")
        for chunk in ("5", "100000", "1", "0"):                            # 100000: clamped to 4096; 0: taken as 1
            if chunk in ("1", "0") and name != "ties_u8":                  # (a launch per query: on the three queries of ties_u8 alone)
                continue
            monkeypatch.setenv("BANG_SCAN_QUERY_CHUNK", chunk)
            _same(e.scan(q, 10), want[10], (name, "chunk", chunk))
        monkeypatch.setenv("BANG_SCAN_STRIPES", "7")
        monkeypatch.setenv("BANG_SCAN_QUERY_CHUNK", "5")
        lab, a, b = SI.label_case("rand4", "mixed", ix, q.shape[0], d)
        e.set_labels(lab)
        _same(e.scan(q, 10, a, b), SR.answer(d, 10, labels=lab, any_=a, all_=b), (name, "filters across chunks"))


@pytest.mark.parametrize("name", ["small_u8", "small_i8", "small_f32"])
def test_host_placement_scans_the_vector_table(request, name):
    """graph = host with pull = 1: the vectors come from the packed table d_vecs at vec_bytes"""
    import bang_amd
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    x = SI.excl_edges(ix.N)
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1) as e:
        _same(e.scan(q, 10), SR.answer(d, 10), (name, "host"))
        e.set_excluded(x)
        _same(e.scan(q, 100), SR.answer(d, 100, excluded=x), (name, "host, excluded"))
        e.set_searchparams(10, 48)                                         # ... and with a live allocation
        e.alloc(q.shape[0])
        e.init(q.shape[0])
        _same(e.scan(q, 10), SR.answer(d, 10, excluded=x), (name, "host, allocated"))
        e.query(q)
        e.free()


@pytest.mark.parametrize("case", ["i8_a12", "u8_a12", "f32_a12"])
def test_after_an_insert_the_scan_covers_the_new_ids(case):
    ix, v, Lb, alpha = I.case(case)
    q = np.ascontiguousarray(np.concatenate([I.get(I.CASES[case][0])[1][:12], v[:12]]))      # the index's queries and vectors that were inserted
    with _engine(ix, capacity=ix.N + len(v)) as e:
        before = e.scan(q, 10)
        assert (before[2] == ix.N).all()
        assert e.insert(v, Lb, alpha) == ix.N
        got = e.scan(q, 10)
        exported = e.export_index(ix)
    assert exported.N == ix.N + len(v)
    _same(got, SR.answer(SR.distances(exported, q), 10), case)
    assert (got[2] == exported.N).all() and (got[0][12:] >= ix.N).any() and (got[1][0, 12:] == 0).all(), "an inserted vector is not at distance 0 of itself"
    _same(before, SR.answer(SR.distances(exported, q), 10, n_nodes=ix.N), (case, "before"))


@pytest.mark.parametrize("case", ["i8_ball24", "i8_ball8_med", "deep_ball4"])
def test_after_a_consolidation_no_removed_id_is_returned(case):
    ix, x, alpha = CI.case(case)
    gone = x[x != ix.medoid]
    qsrc = I.get(CI.CASES[case][0])[1] if CI.CASES[case][0] in I.INDEXES else ix.vectors()[:8]
    q = np.ascontiguousarray(np.concatenate([qsrc[:8], ix.vectors()[gone[:8]]]))
    d = SR.distances(ix, q)
    with _engine(ix, capacity=ix.N) as e:
        e.set_excluded(x)
        _same(e.scan(q, 10), SR.answer(d, 10, excluded=x), (case, "excluded, before"))
        e.consolidate(alpha)
        got = e.scan(q, 10)
        assert not np.isin(got[0], gone).any(), "a removed id was returned"
        medoid_in = bool((x == ix.medoid).any())
        assert (got[2] == ix.N - len(gone) - (1 if medoid_in else 0)).all()
        _same(got, SR.answer(d, 10, excluded=x), (case, "after"))          # X & {med} stays excluded, D is removed: the same candidates
        e.clear_excluded()                                                 # the medoid is live again; the removed nodes are not
        _same(e.scan(q, 10), SR.answer(d, 10, removed=gone), (case, "cleared"))
        e.consolidate(alpha)                                               # nothing to fold: the removed set stays
        _same(e.scan(q, 128), SR.answer(d, 128, removed=gone), (case, "second consolidation"))
        exported = e.export_index(ix)
    with _engine(exported) as f:                                           # the bitmap is not persisted: a reloaded index is scanned whole
        got = f.scan(q, 10)
        assert (got[2] == ix.N).all() and np.isin(got[0], gone).any()


def test_truth_tool_writes_what_the_scan_returns(request, tmp_path, monkeypatch):
    from bang_amd import formats, truth
    ix, q = _input(request, "small_i8")
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    x = SI.excl_edges(ix.N)
    formats.write_bin(str(tmp_path / "x.bin"), x.reshape(-1, 1).astype(np.uint32))
    d = SR.distances(ix, q)
    for excl in (None, x):
        if excl is not None:
            monkeypatch.setenv("BANG_EXCLUDE_FILE", str(tmp_path / "x.bin"))
        out = str(tmp_path / "truth.bin")
        assert truth.main([prefix, str(tmp_path / "q.bin"), "100", out]) == 0
        ids, dists = formats.read_truthset(out)
        want = SR.answer(d, 100, excluded=excl)
        assert np.array_equal(ids.astype(np.uint64), want[0]) and np.array_equal(dists.view(np.uint32), np.ascontiguousarray(want[1].T).view(np.uint32))


def test_refused_calls_leave_the_engine_serving(request):
    import bang_amd
    ix, q = _input(request, "small_f32")
    d = SR.distances(ix, q)
    with _engine(ix) as e:
        e.set_searchparams(10, 48)
        e.alloc(q.shape[0])
        e.init(q.shape[0])
        first = e.query(q)
        with pytest.raises(bang_amd.BangError, match=r"k = 129"):
            e.scan(q, 129)
        with pytest.raises(bang_amd.BangError, match=r"k = 0"):
            e.scan(q, 0)
        bad = q.copy()
        bad[3, 5] = np.nan
        with pytest.raises(bang_amd.BangError, match=r"query 3, dimension 5"):
            e.scan(bad, 10)
        a = np.zeros(q.shape[0], np.uint32)
        with pytest.raises(bang_amd.BangError, match=r"exactly one of any / all"):
            e.scan(q, 10, any=a)
        with pytest.raises(bang_amd.BangError, match=r"labels"):
            e.scan(q, 10, a, a)
        e.init(q.shape[0])
        again = e.query(q)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
        _same(e.scan(q, 10), SR.answer(d, 10), "after the refusals")
        e.free()
        e.set_searchparams(10, 48, bang_amd.DIST_MIPS)
        with pytest.raises(bang_amd.BangError, match=r"MIPS"):
            e.scan(q, 10)


def test_refusals_of_what_the_scan_cannot_read(request):
    import bang_amd
    ix, q = _input(request, "small_f32")
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"fp16"):
            e.scan(q, 10)
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=0, vectors=0) as e:
        with pytest.raises(bang_amd.BangError, match=r"no resident vectors"):
            e.scan(q, 10)
    wide, wq = ST.get("u8_48")
    with _engine(wide) as e:
        with pytest.raises(bang_amd.BangError, match=r"bang_search_can_rerank"):
            e.scan(wq, 10)


# ---------------------------------------------------------------------------------------------------------------------
# bang_scan_e itself, through ctypes: every refusal on a LOADED engine with its code, its message, sentinel-filled output buffers and times
# ---------------------------------------------------------------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5


class _Raw:
    """bang_scan_e on the handle of an Engine with caller-owned, sentinel-filled outputs"""

    def __init__(self, e, Q, k):
        from bang_amd import binding as B
        self.e, self.lib = e, B.lib()
        self.lib.bang_scan_e.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.ids = np.full((Q, k), 0x7777777777777777, np.uint64)
        self.dists = np.full((k, Q), 7.5, np.float32)
        self.matched = np.full(Q, 0x77777777, np.uint32)

    def refused(self, code, word, q, nq, k, any_=None, all_=None, ids="own", dists="own", matched="own"):
        p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        own = dict(ids=self.ids, dists=self.dists, matched=self.matched)
        ids, dists, matched = (own[n] if v == "own" else v for n, v in (("ids", ids), ("dists", dists), ("matched", matched)))
        rc = self.lib.bang_scan_e(self.e._h, p(q), nq, k, p(any_), p(all_), p(ids), p(dists), p(matched))
        msg = self.lib.bang_last_error().decode()
        assert rc == code and "bang_scan" in msg and word in msg, (rc, msg, word)
        assert (self.ids == 0x7777777777777777).all() and (self.dists == 7.5).all() and (self.matched == 0x77777777).all(), ("a refused call wrote an output", word)
        assert self.e.scan_times() == dict(scan=0, merge=0, total=0), ("a refused call left times", word)


def test_every_refusal_of_bang_scan_e_on_a_loaded_engine(request):
    """code, message, untouched sentinel-filled buffers and zero times for each refusal; then the same engines answer"""
    import bang_amd
    ix, q = _input(request, "small_f32")
    Q, k = q.shape[0], 10
    q = np.ascontiguousarray(q)
    d = SR.distances(*_input(request, "small_f32"))
    words = np.zeros(Q, np.uint32)
    bad = q.copy()
    bad[Q - 1, ix.D - 1] = np.inf
    with _engine(ix) as e:
        r = _Raw(e, Q, k)
        r.refused(ERR_ARG, "queries are null", None, Q, k)
        r.refused(ERR_ARG, "output buffer", q, Q, k, ids=None)
        r.refused(ERR_ARG, "output buffer", q, Q, k, dists=None)
        r.refused(ERR_ARG, "nq = 0", q, 0, k)
        r.refused(ERR_ARG, "nq = %d" % ((1 << 20) + 1), q, (1 << 20) + 1, k)
        r.refused(ERR_ARG, "k = 0", q, Q, 0)
        r.refused(ERR_ARG, "k = 129", q, Q, 129)
        r.refused(ERR_ARG, "exactly one of any / all", q, Q, k, any_=words)
        r.refused(ERR_ARG, "exactly one of any / all", q, Q, k, all_=words)
        r.refused(ERR_ARG, "labels", q, Q, k, any_=words, all_=words)
        r.refused(ERR_ARG, "query %d, dimension %d" % (Q - 1, ix.D - 1), bad, Q, k)
        e.set_searchparams(10, 48, bang_amd.DIST_MIPS)
        r.refused(ERR_UNSUPPORTED, "MIPS", q, Q, k)
        e.set_searchparams(10, 48)
        rc = r.lib.bang_scan_e(e._h, q.ctypes.data, Q, k, None, None, r.ids.ctypes.data, r.dists.ctypes.data, None)      # matched may be NULL
        assert rc == 0, r.lib.bang_last_error().decode()
        want = SR.answer(d, k)
        assert np.array_equal(r.ids, want[0]) and np.array_equal(r.dists.view(np.uint32), want[1].view(np.uint32)) and (r.matched == 0x77777777).all()
        assert e.scan_times()["total"] > 0
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1, vectors_fp16=1) as e:
        _Raw(e, Q, k).refused(ERR_UNSUPPORTED, "fp16", q, Q, k)
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=0, vectors=0) as e:
        _Raw(e, Q, k).refused(ERR_UNSUPPORTED, "no resident vectors", q, Q, k)
    wide, wq = ST.get("u8_48")
    with _engine(wide) as e:
        _Raw(e, wq.shape[0], k).refused(ERR_UNSUPPORTED, "bang_search_can_rerank", np.ascontiguousarray(wq), wq.shape[0], k)
