"""The exact range scan on the GPU (bang_scan_range_e, bang_k_scan_range; DESIGN.md section 2 CANON 26): lims, ids, distance bits, offered and matched
compared bit for bit with tests/scan_range_reference.py (scan_reference's distances and masks, the compare, the first max_hits in id order, np.sort)."""
import ctypes as C

import numpy as np
import pytest

import anydim_inputs as A
import scan_inputs as SI
import scan_range_reference as RR
import scan_reference as SR
import test_gpu_scan_any as TA

pytestmark = pytest.mark.gpu

LAYOUTS = SI.FIXTURES + ("u8_16", "u8_32", "i8_256", "i8_100", "f32_67")        # half a k-step, one, eight; the short last k-step; an odd float D
HITS = (1, 64, 65, 4096)


def _input(request, name):
    """-> (Index, queries)"""
    if name in SI.FIXTURES:
        return request.getfixturevalue(name)[:2]
    if name in SI.SMALL:
        return SI.small(name)
    return A.get(name)


def _engine(ix, **opts):
    import bang_amd
    opts.setdefault("graph", bang_amd.GRAPH_DEVICE)
    e = bang_amd.Engine(ix.dtype, **opts)
    e.load_index(ix)
    return e


def _same(got, want, what):
    assert RR.first_difference(got, want) == "equal", (what, RR.first_difference(got, want))


@pytest.mark.parametrize("name", LAYOUTS)
def test_every_layout_at_every_radius(request, name):
    ix, q = _input(request, name)
    d = SR.distances(ix, q)
    Q = q.shape[0]
    mixed = np.array([np.inf, 0.0, -1.0, np.nan], np.float32)[np.arange(Q) % 4]
    assert ix.N < 4096
    with _engine(ix) as e:
        for hits in HITS:
            for rank in (0, 9, 99):
                _same(e.scan_range(q, RR.rank_radii(d, rank), hits), RR.answer(d, RR.rank_radii(d, rank), hits), (name, hits, rank))
            got = e.scan_range(q, mixed, hits)
            _same(got, RR.answer(d, mixed, hits), (name, hits, "inf, 0, -1, NaN"))
            cnt = np.diff(got[0].astype(np.int64))
            assert (cnt[0::4] == min(hits, ix.N)).all() and (got[3][0::4] == ix.N).all() and (cnt[2::4] == 0).all() and (cnt[3::4] == 0).all()
        got = e.scan_range(q, RR.rank_radii(d, 99), 64)
        assert (got[3] >= 100).all() and (np.diff(got[0].astype(np.int64)) == 64).all(), "the rank-99 radius does not truncate at 64"
        t, tr = e.scan_times(), e.scan_range_times()
        assert t["total"] > 0 and tr["count"] > 0 and tr["emit"] > 0 and abs(t["scan"] - tr["count"] - tr["emit"]) < 1e-6


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_ties_keep_the_lowest_ids(kind):
    ix, q, tied = SI.ties(kind)
    d = SR.distances(ix, q)
    rad = np.ascontiguousarray(d[:, int(tied[0])])                          # the tie group's distance: the 50 copies and nothing else
    with _engine(ix) as e:
        for hits in (10, 64):
            got = e.scan_range(q, rad, hits)
            _same(got, RR.answer(d, rad, hits), (kind, hits))
            assert (got[3] == 50).all()
            for i in range(q.shape[0]):
                assert np.array_equal(got[1][int(got[0][i]):int(got[0][i + 1])], tied[:min(hits, 50)]), (kind, hits, i)


def test_sums_on_both_sides_of_2_pow_24():
    """ten points far below 2^24, 290 near 5.9e7: a radius below 2^24, one between the groups (>= 2^24: the chain is evaluated and refuses), one
    above the far group, whose answer holds distances that are NOT float32(integer sum)"""
    ix, q = TA._get("handover")
    d = TA._dist("handover")
    v, qq = ix.vectors().astype(np.int64), q.astype(np.int64)
    plain = np.array([[((v[x] - qq[i]) ** 2).sum() for x in range(ix.N)] for i in range(q.shape[0])], np.int64).astype(np.float32)
    assert (plain.view(np.uint32) != d.view(np.uint32)).any(), "the input does not tell the chain from the integer's float image"
    near, far = d[:, list(TA.HAND_NEAR)].max(), np.delete(d, list(TA.HAND_NEAR), axis=1)
    assert near < 1.0e6 < 2.0 ** 25 < far.min() and far.max() < 1.0e9
    with _engine(ix) as e:
        for rad, n in ((1.0e6, 10), (2.0 ** 25, 10), (1.0e9, 300)):
            got = e.scan_range(q, np.float32(rad), 4096)
            _same(got, RR.answer(d, np.full(q.shape[0], rad, np.float32), 4096), rad)
            assert (got[3] == n).all()


def _k_range(ix, d_vec, stride, q, rad, n_nodes, hits, runs):
    """-> (the packed answer, the geometry's maximum of runs)"""
    from bang_amd import binding as B
    lib, Q = B.lib(), q.shape[0]
    lib.bang_scan_range_geometry.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    t, r, most = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.bang_scan_range_geometry(B.DTYPE_CODE[ix.dtype], ix.D, Q, n_nodes, C.byref(t), C.byref(r), C.byref(most)) == 0
    runs = min(runs, most.value)
    nbytes = 4 * Q * max(runs, r.value)
    bufs = dict(q=B.DeviceBuffer.from_numpy(np.ascontiguousarray(q)), rad=B.DeviceBuffer.from_numpy(np.ascontiguousarray(rad, np.float32)),
                scratch=B.DeviceBuffer(nbytes), ids=B.DeviceBuffer(Q * hits * 4), dists=B.DeviceBuffer(Q * hits * 4), words=B.DeviceBuffer(3 * Q * 4))
    p = B.ScanRangeParams()
    p.d_vec_base, p.vec_stride, p.dtype, p.D, p.n_nodes = d_vec, stride, B.DTYPE_CODE[ix.dtype], ix.D, n_nodes
    p.d_queries, p.nq, p.d_radius, p.max_hits, p.runs = bufs["q"].ptr, Q, bufs["rad"].ptr, hits, runs
    p.d_scratch, p.scratch_bytes, p.d_hit_ids, p.d_hit_dists = bufs["scratch"].ptr, nbytes, bufs["ids"].ptr, bufs["dists"].ptr
    p.d_offered, p.d_count, p.d_matched = bufs["words"].ptr, bufs["words"].ptr + 4 * Q, bufs["words"].ptr + 8 * Q
    lib.bang_k_scan_range.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.bang_k_scan_range(C.byref(p), None) == 0, lib.bang_last_error().decode()
    B.sync()
    offered, count, matched = bufs["words"].download(np.uint32, (3, Q))
    ids, dists = bufs["ids"].download(np.uint32, (Q, hits)), bufs["dists"].download(np.float32, (Q, hits))
    for b in bufs.values():
        b.free()
    keep = np.arange(hits)[None, :] < count[:, None]
    lims = np.zeros(Q + 1, np.uint64)
    np.cumsum(count, dtype=np.uint64, out=lims[1:])
    return (lims, ids[keep].astype(np.uint64), dists[keep], offered, matched), most.value


@pytest.mark.parametrize("name,QS", [("small_u8", (1, 31, 33)), ("small_f32", (1, 15, 17))])
def test_kernel_entry_on_prefixes(request, name, QS):
    """n_nodes = 1 .. 65 and N, query tiles that end inside a tile, runs = 1, 3 and the most a launch accepts: the answer does not depend on runs"""
    from bang_amd import binding as B
    ix, q = _input(request, name)
    d0 = SR.distances(ix, q)
    graph = B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.graph), slack=256)
    try:
        for Q in QS:
            qq, d = SI.queries_of(q, Q), SI.tile_dist(d0, Q)
            rad = RR.rank_radii(d, 9)
            for n in SI.N_PREFIXES + (ix.N,):
                want = RR.answer(d, rad, 64, n_nodes=n)
                _, most = _k_range(ix, graph.ptr, ix.entry_len, qq, rad, n, 64, 1)
                for runs in sorted({1, min(3, most), most}):
                    _same(_k_range(ix, graph.ptr, ix.entry_len, qq, rad, n, 64, runs)[0], want, (name, Q, n, runs))
    finally:
        graph.free()


@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_masks(request, name):
    ix, q = _input(request, name)
    d, Q = SR.distances(ix, q), q.shape[0]
    rad, x = RR.rank_radii(d, 99), SI.excl_edges(ix.N)
    with _engine(ix, capacity=ix.N) as e:
        for table, batch in (("nobody", "bit31"), ("rand4", "mixed")):
            lab, a, b = SI.label_case(table, batch, ix, Q, d)
            e.set_labels(lab)
            got = e.scan_range(q, rad, 4096, a, b)
            _same(got, RR.answer(d, rad, 4096, labels=lab, any_=a, all_=b), (name, table, batch))
            assert np.array_equal(got[4], SR.candidates(ix.N, Q, labels=lab, any_=a, all_=b).sum(axis=1))
        e.set_excluded(x)
        _same(e.scan_range(q, rad, 4096), RR.answer(d, rad, 4096, excluded=x), (name, "excluded"))
        e.consolidate(1.2)                                                 # X \ {medoid} is removed, X & {medoid} stays excluded: the same candidates
        got = e.scan_range(q, np.inf, 4096)
        _same(got, RR.answer(d, np.full(Q, np.inf, np.float32), 4096, excluded=x), (name, "removed"))
        e.clear_excluded()
        gone = x[x != ix.medoid]
        _same(e.scan_range(q, rad, 65, a, b), RR.answer(d, rad, 65, removed=gone, labels=lab, any_=a, all_=b), (name, "removed, filters"))


def test_host_placement_scans_the_vector_table(small_u8):
    import bang_amd
    ix, q = small_u8[:2]
    d = SR.distances(ix, q)
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1) as e:
        for rank, hits in ((9, 64), (99, 64), (99, 4096)):
            _same(e.scan_range(q, RR.rank_radii(d, rank), hits), RR.answer(d, RR.rank_radii(d, rank), hits), (rank, hits))


def test_refusals_name_their_reason_and_the_engine_still_serves(small_f32):
    import bang_amd
    ix, q = small_f32[:2]
    d = SR.distances(ix, q)
    rad = RR.rank_radii(d, 9)
    with _engine(ix) as e:
        e.set_searchparams(10, 48, bang_amd.DIST_MIPS)
        with pytest.raises(bang_amd.BangError, match=r"code -5.*MIPS"):
            e.scan_range(q, rad, 64)
        e.set_searchparams(10, 48)
        with pytest.raises(bang_amd.BangError, match=r"code -1.*nq x max_hits"):
            e.scan_range(np.zeros(((1 << 16) + 1, ix.D), np.float32), 1.0, 4096)
        with pytest.raises(bang_amd.BangError, match=r"max_hits = 4097"):
            e.scan_range(q, rad, 4097)
        _same(e.scan_range(q, rad, 64), RR.answer(d, rad, 64), "after the refusals")
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1, vectors_fp16=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"code -5.*fp16"):
            e.scan_range(q, rad, 64)
