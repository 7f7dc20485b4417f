"""Inserts on a GPU (csrc/bang_insert.hip, bang_insert_e), bit for bit against tests/insert_reference.py: bang_k_prune on lists of 0 .. 512
entries, bang_k_pq_encode on the four pivot layouts, and the engine -- entries and codes after one and two batches, an engine loaded from the
export against the engine that inserted, an excluded inserted id, and the refusals."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import insert_inputs as I
import insert_reference as IR
from exact_reference import Reference

pytestmark = pytest.mark.gpu

K = 10
LENGTHS = (0, 1, 63, 64, 65, 512)
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(name):
    if name not in _CACHE:
        _CACHE[name] = Reference(I.get(name)[0])
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------------------------
# bang_k_prune
# ---------------------------------------------------------------------------------------------------------------------
def _make_list(ref, rng, node, length, pool=None):
    """An ordered candidate list of `length` distinct ids around `node`: ascending exact distance to its vector, as a worklist is."""
    pool = ref.ix.N if pool is None else pool
    ids = rng.choice(pool, length, replace=False).astype(np.uint32)
    d = ref.exact(ids, IR.vector_of(ref, node))
    o = np.argsort(d, kind="stable")
    return ids[o], d[o]


def _prune_gpu(ix, lists, owns, R, alpha, graph_ptr=None, entry_len=None, n_nodes=None, max_wgs=0, max_waves=0, stride=None):
    """-> (rows u32 [n_lists][R + 1], abort word)"""
    from bang_amd import binding as B
    n = len(lists)
    stride = stride or max(1, max(len(l[0]) for l in lists))
    ids = np.zeros((n, stride), np.uint32)
    d = np.zeros((n, stride), np.float32)
    cnt = np.zeros(n, np.uint32)
    for i, (a, b) in enumerate(lists):
        ids[i, :len(a)], d[i, :len(a)], cnt[i] = a, b, len(a)
    keep = []
    if graph_ptr is None:
        g = B.DeviceBuffer.from_numpy(ix.graph, slack=256)
        keep.append(g)
        graph_ptr, entry_len = g.ptr, ix.entry_len
    bufs = [B.DeviceBuffer.from_numpy(x) for x in (ids, d, cnt, np.asarray(owns, np.uint32))]
    out = B.DeviceBuffer(n * (R + 1) * 4)
    out.upload(np.full(n * (R + 1), 0xABABABAB, np.uint32))
    ab = B.DeviceBuffer(4)
    p = B.PruneParams()
    p.d_graph, p.entry_len, p.dtype, p.D, p.n_nodes, p.R = graph_ptr, entry_len, B.DTYPE_CODE[ix.dtype], ix.D, n_nodes or ix.N, R
    p.alpha2, p.n_lists, p.list_stride = float(IR.alpha2_of(alpha)), n, stride
    p.d_list_ids, p.d_list_dists, p.d_list_cnt, p.d_own = (b.ptr for b in bufs)
    p.d_out, p.out_stride, p.out_by_own, p.max_wgs, p.max_waves, p.d_abort = out.ptr, 4 * (R + 1), 0, max_wgs, max_waves, ab.ptr
    fn = B.lib().bang_k_prune
    fn.argtypes = [C.c_void_p, C.c_void_p]
    B._check(fn(C.byref(p), None), "bang_k_prune")
    B.sync()
    rows, abort = out.download(np.uint32, (n, R + 1)), int(ab.download(np.uint32, (1,))[0])
    for b in bufs + keep + [out, ab]:
        b.free()
    return rows, abort


def _want_rows(ref, lists, owns, R, alpha):
    rows = np.zeros((len(lists), R + 1), np.uint32)
    for i, (a, b) in enumerate(lists):
        r = IR.prune(ref, int(owns[i]), a, b, R, IR.alpha2_of(alpha))
        rows[i, 0] = len(r)
        rows[i, 1:1 + len(r)] = r
    return rows


@pytest.mark.parametrize("alpha", [1.2, 8.0])
@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("name", ["i8", "u8", "deep", "f32"])
def test_prune_every_length(name, R, alpha):
    """lists of 0, 1, 63, 64, 65 and 512 entries, three of each, one with its own id inside; 8 waves in 4 workgroups of two take 19 lists:
    every wave takes a second list and the last round leaves workgroups partly idle"""
    ref = _ref(name)
    ix = ref.ix
    rng = np.random.default_rng(R + int(alpha * 10) + ix.D)
    lists, owns = [], []
    for length in LENGTHS:
        for _ in range(3):
            node = int(rng.integers(ix.N))
            lists.append(_make_list(ref, rng, node, length))
            owns.append(node)
    lists.append(_make_list(ref, rng, 5, 100))
    owns.append(int(lists[-1][0][3]))                                      # its own id inside the list
    assert len(lists) == 19
    want = _want_rows(ref, lists, owns, R, alpha)
    assert (want[:, 0] == R).any() or alpha < 8.0
    got, abort = _prune_gpu(ix, lists, owns, R, alpha, max_wgs=4, max_waves=2)
    assert abort == 0
    assert np.array_equal(got, want)
    assert owns[-1] not in got[-1, 1:1 + got[-1, 0]]


def test_prune_partial_last_workgroup_and_default_geometry():
    ref = _ref("u8")
    ix = ref.ix
    rng = np.random.default_rng(99)
    lists = [_make_list(ref, rng, int(t), 70 + 9 * i) for i, t in enumerate(rng.integers(ix.N, size=7))]
    owns = [ix.N] * 7                                                       # (no own node: an id no list holds)
    want = _want_rows(ref, lists, owns, ix.R, 1.2)
    for wgs, waves in ((4, 2), (0, 0), (1, 1)):                           # 4 x 2 waves for 7 lists; the launch's own geometry; one wave takes all 7
        got, abort = _prune_gpu(ix, lists, owns, ix.R, 1.2, max_wgs=wgs, max_waves=waves)
        assert abort == 0 and np.array_equal(got, want), (wgs, waves)


@pytest.mark.parametrize("name", ["i8", "f32"])
def test_prune_id_outside_the_index_ends_the_list(name):
    ref = _ref(name)
    ix = ref.ix
    rng = np.random.default_rng(5)
    lists = [_make_list(ref, rng, 11, 90), _make_list(ref, rng, 12, 130), _make_list(ref, rng, 13, 40)]
    bad = [(lists[0][0].copy(), lists[0][1]), (lists[1][0].copy(), lists[1][1]), lists[2]]
    bad[0][0][70] = ix.N                                                   # the first id outside: never dereferenced
    bad[1][0][0] = 0xFFFFFFFF                                              # at the head: an empty list
    owns = [ix.N + 1] * 3
    cut = [(lists[0][0][:70], lists[0][1][:70]), (lists[1][0][:0], lists[1][1][:0]), lists[2]]
    got, abort = _prune_gpu(ix, bad, owns, ix.R, 1.2)
    assert abort == 2
    assert np.array_equal(got, _want_rows(ref, cut, owns, ix.R, 1.2))
    # a skipped list leaves its row alone
    from bang_amd import binding as B
    got, abort = _prune_gpu(ix, lists, [ix.N, 0xFFFFFFFF, ix.N], ix.R, 1.2)
    assert abort == 0 and (got[1] == 0xABABABAB).all() and got[0, 0] > 0 and got[2, 0] > 0
    assert B.device_count() >= 1


@pytest.mark.parametrize("name", ["i8_64_m16", "f32_128_m32"])
def test_prune_row_addressing_beyond_4_gib(name):
    """the graph entries 32 MiB apart: id * entry_len passes 4 GiB at id 128; 200 entries, lists over all of them"""
    import stretch_inputs as S
    ix, _ = S.get(name)
    NN = 200
    stride = S.stride_of(ix.entry_len)
    assert (NN - 1) * stride > (4 << 30) and stride % 4 == 0
    buf, ptr = S.stretched(ix.graph[:NN], stride)
    ref = Reference(ix)
    rng = np.random.default_rng(17)
    lists = [_make_list(ref, rng, int(t), n, pool=NN) for t, n in ((3, 64), (150, 120), (199, 200), (130, 1))]
    assert all((l[0] >= 128).any() for l in lists)
    owns = [3, 150, 199, 130]
    want = _want_rows(ref, lists, owns, ix.R, 1.2)
    got, abort = _prune_gpu(ix, lists, owns, ix.R, 1.2, graph_ptr=ptr, entry_len=stride, n_nodes=NN)
    buf.free()
    assert abort == 0 and np.array_equal(got, want)
    picked = np.concatenate([want[i, 1:1 + want[i, 0]] for i in range(len(lists))])
    assert (picked >= 128).any(), "no picked candidate lies beyond 4 GiB: its vector is what a wrapped offset would miss"


# ---------------------------------------------------------------------------------------------------------------------
# bang_k_worklist_lists, bang_k_backedge
# ---------------------------------------------------------------------------------------------------------------------
def test_worklist_lists_cut_at_the_first_pad_entry():
    """hand-made worklists of L = 70: no pad, a pad at the head, at the piece boundary (64), in the middle with entries behind it, at the last place"""
    from bang_amd import binding as B
    L, Q, stride, MARK = 70, 5, 72, 0xCDCDCDCD
    pads = [L, 0, 64, 33, 69]
    rng = np.random.default_rng(3)
    wl = rng.integers(0, 1 << 31, (Q, L)).astype(np.uint64)
    wd = np.sort(rng.random((L, Q)).astype(np.float32), axis=0)             # rank-major
    for q, p in enumerate(pads):
        if p < L:
            wl[q, p] = np.uint64(0xFFFFFFFFFFFFFFFF)                          # what stands behind the first pad entry is never read as an id
    bufs = [B.DeviceBuffer.from_numpy(wl), B.DeviceBuffer.from_numpy(wd)]
    outs = [B.DeviceBuffer.from_numpy(np.full(n, MARK, np.uint32)) for n in (Q * stride, Q * stride, Q)]
    fn = B.lib().bang_k_worklist_lists
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    B._check(fn(bufs[0].ptr, bufs[1].ptr, L, 0, Q, Q, outs[0].ptr, outs[1].ptr, stride, outs[2].ptr, None), "bang_k_worklist_lists")
    B.sync()
    ids, d, cnt = outs[0].download(np.uint32, (Q, stride)), outs[1].download(np.uint32, (Q, stride)), outs[2].download(np.uint32, (Q,))
    for b in bufs + outs:
        b.free()
    assert list(cnt) == pads
    for q, p in enumerate(pads):
        assert np.array_equal(ids[q, :p], wl[q, :p].astype(np.uint32)) and np.array_equal(d[q, :p], _bits(wd[:p, q])), q
        assert (ids[q, p:] == MARK).all() and (d[q, p:] == MARK).all(), (q, "written at or behind the pad")


def _backedge_gpu(ix, graph, n_nodes, targets, incoming):
    """-> (graph after, cand ids, cand distance bits, offered, own_out, stats, abort)"""
    from bang_amd import binding as B
    T = len(targets)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in incoming])]).astype(np.uint32)
    srcs = np.concatenate(incoming).astype(np.uint32)
    g = B.DeviceBuffer.from_numpy(graph, slack=256)
    ins = [B.DeviceBuffer.from_numpy(x) for x in (np.asarray(targets, np.uint32), offs, srcs)]
    MARK = 0xCDCDCDCD
    outs = [B.DeviceBuffer.from_numpy(np.full(n, MARK, np.uint32)) for n in (T * 512, T * 512, T, T)]
    ctl = B.DeviceBuffer(16)
    p = B.BackedgeParams()
    p.d_graph, p.entry_len, p.dtype, p.D, p.R, p.n_nodes, p.n_old, p.n_targets = g.ptr, ix.entry_len, B.DTYPE_CODE[ix.dtype], ix.D, ix.R, n_nodes, ix.N, T
    p.d_targets, p.d_offs, p.d_srcs = (b.ptr for b in ins)
    p.d_cand_ids, p.d_cand_dists, p.d_offered, p.d_own_out = (b.ptr for b in outs)
    p.d_stats, p.d_abort = ctl.ptr, ctl.ptr + 12
    fn = B.lib().bang_k_backedge
    fn.argtypes = [C.c_void_p, C.c_void_p]
    B._check(fn(C.byref(p), None), "bang_k_backedge")
    B.sync()
    c = ctl.download(np.uint32, (4,))
    res = (g.download(np.uint8, graph.shape), outs[0].download(np.uint32, (T, 512)), outs[1].download(np.uint32, (T, 512)),
           outs[2].download(np.uint32, (T,)), outs[3].download(np.uint32, (T,)), list(c[:3]), int(c[3]))
    for b in [g, ctl] + ins + outs:
        b.free()
    return res


@pytest.mark.parametrize("name", ["i8", "f32"])
def test_backedge_appends_overflows_and_never_follows_an_id_outside_the_index(name):
    """hand-made targets: a row with room for exactly its three new ids; a full row (old row ++ new ids and their exact distances to the target's
    vector); a target that is not an old node; an old row that holds an id outside the index"""
    ix, _ = I.get(name)
    R, N, vb = ix.R, ix.N, ix.D * (4 if ix.dtype == "float" else 1)
    new = I.batch(ix, 16, 55)
    deg0 = np.zeros(16, np.uint32)
    from bang_amd import formats
    graph = np.concatenate([ix.graph, formats.pack_graph(new, deg0, np.zeros((16, R), np.uint32))])
    rows = graph[:, vb:].view(np.uint32)                                   # [N + 16][1 + R], a view
    full = np.flatnonzero(rows[:N, 0] == R)
    t0, t1, t3 = (int(x) for x in full[:3])
    rows[t0, 0] = R - 3
    rows[t0, 1 + R - 3:] = 0
    bad_at = 5
    rows[t3, 1 + bad_at] = N + 16 + 7                                      # an id >= n_nodes inside an old row
    before = graph.copy()
    inc = [np.array([N + 1, N + 4, N + 9]), np.array([N + 2, N + 3]), np.array([N + 5]), np.array([N, N + 15])]
    targets = [t0, t1, N + 1, t3]
    ref = Reference(dataclasses.replace(ix, N=N + 16, graph=before, codes=np.zeros((N + 16, ix.m), np.uint8)))
    SKIP, MARK = 0xFFFFFFFF, 0xCDCDCDCD
    for upto, want_abort in ((2, 0), (4, 2)):                              # the two sound targets alone, then all four
        after, ci, cd, offered, own, stats, abort = _backedge_gpu(ix, before, N + 16, targets[:upto], inc[:upto])
        assert abort == want_abort
        want = before.copy()
        wrows = want[:, vb:].view(np.uint32)
        wrows[t0, 1 + R - 3: 1 + R] = inc[0]
        wrows[t0, 0] = R
        assert np.array_equal(after, want), "only the appended row changes; no other byte of the table does"
        assert offered[0] == 0 and own[0] == SKIP and (ci[0] == MARK).all()
        cand = np.concatenate([before[t1, vb:].view(np.uint32)[1:1 + R], inc[1]]).astype(np.uint32)
        assert offered[1] == R + 2 and own[1] == t1 and np.array_equal(ci[1, :R + 2], cand) and (ci[1, R + 2:] == MARK).all()
        assert np.array_equal(cd[1, :R + 2], _bits(ref.exact(cand, IR.vector_of(ref, t1))))
        if upto == 4:
            assert offered[2] == 0 and own[2] == SKIP and (ci[2] == MARK).all()          # not an old node: skipped
            head = before[t3, vb:].view(np.uint32)[1:1 + bad_at]
            assert offered[3] == bad_at and own[3] == t3 and np.array_equal(ci[3, :bad_at], head)  # the list ends in front of the id
            assert np.array_equal(cd[3, :bad_at], _bits(ref.exact(head, IR.vector_of(ref, t3))))
        assert stats == [1, 1 if upto == 2 else 2, 0]


# ---------------------------------------------------------------------------------------------------------------------
# bang_k_pq_encode
# ---------------------------------------------------------------------------------------------------------------------
def _encode_gpu(ix, v, lut_points, code_stride):
    from bang_amd import binding as B
    n = v.shape[0]
    bufs = [B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.pivots.T, np.float32)), B.DeviceBuffer.from_numpy(v, slack=256),
            B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.centroid, np.float32)), B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.chunk_off, np.uint32)),
            B.DeviceBuffer(lut_points * ix.m * 256 * 4)]
    out = B.DeviceBuffer(n * code_stride + 256)
    out.upload(np.full(n * code_stride + 256, 0xEE, np.uint8))
    fn = B.lib().bang_k_pq_encode
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                   C.c_void_p, C.c_uint64, C.c_void_p]
    B._check(fn(bufs[0].ptr, bufs[1].ptr, B.DTYPE_CODE[ix.dtype], bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, lut_points, n, ix.D, ix.m, out.ptr, code_stride,
                None), "bang_k_pq_encode")
    B.sync()
    raw = out.download(np.uint8, (n * code_stride + 256,))
    for b in bufs + [out]:
        b.free()
    assert (raw[n * code_stride:] == 0xEE).all(), "bytes behind the last row were written"
    return raw[:n * code_stride].reshape(n, code_stride)


@pytest.mark.parametrize("name", ["i8", "u8", "deep", "f32"])
def test_pq_encode_lowest_argmin(name):
    """m = 16, 70, 74 and 32; two pivots made equidistant from every vector (rows k0 and 255 of the table equal) pin the lowest-k rule; the batch
    runs in chunks of 5 tables; rows at a stride of m and of 128 with their pad bytes 0"""
    ix, _ = I.get(name)
    v = I.batch(ix, 23, 31)
    k0 = int(IR.encode(Reference(ix), v[0])[0])
    hi, lo = (255, k0) if k0 != 255 else (254, 255)
    piv = ix.pivots.copy()
    piv[max(hi, lo)] = piv[min(hi, lo)]
    ix2 = dataclasses.replace(ix, pivots=piv)
    ref = Reference(ix2)
    want = np.stack([IR.encode(ref, x) for x in v])
    lut = ref.orc.lut_build(v[0])
    assert lut[0, min(hi, lo)] == lut[0, max(hi, lo)] == lut[0].min() and want[0, 0] == min(hi, lo)
    assert not (want == max(hi, lo)).any()
    for stride in (ix.m, 128):
        got = _encode_gpu(ix2, v, 5, stride)
        assert np.array_equal(got[:, :ix.m], want), stride
        assert not got[:, ix.m:].any(), "pad bytes of a row are 0"


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def _engine(ix, capacity, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, **(dict(capacity=capacity) if capacity is not None else {}), **opts)
    e.load_index(ix)
    return e


def _search(e, q, L, mode):
    """one batch on a loaded, unallocated engine -> (ids, distance bits, counters); mode: "exact" (distance = 1) or "pq" (the self-paced PQ walk)"""
    e.set_option("distance", 1 if mode == "exact" else 0)
    e.set_option("search", 1)
    e.set_searchparams(K, L)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    out = (ids, _bits(d), e.query_counters(q.shape[0]))
    e.free()
    return out


def _same(a, b, what):
    for x, y, part in zip(a, b, ("ids", "distance bits", "counters")):
        assert np.array_equal(x, y), (what, part)


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_insert_matches_the_reference_byte_for_byte(name):
    ix, v, L, alpha = I.case(name)
    ix2, st = I.reference(name)
    with _engine(ix, ix.N + 200) as e:
        assert e.num_nodes() == ix.N
        assert e.insert(v, L, alpha) == ix.N
        assert e.num_nodes() == ix2.N
        assert np.array_equal(e.entries(0, ix2.N), ix2.graph)
        assert np.array_equal(e.codes(0, ix2.N), ix2.codes)
        s = e.insert_stats()
        assert s == dict(capacity=ix.N + 200, inserted=st["inserted"], backedge_appended=st["appended"], backedge_pruned=st["pruned"],
                         backedge_dropped=st["dropped"])


def test_back_edges_beyond_the_candidate_cap():
    """500 copies of one indexed vector: its node is in every new row, old row ++ 500 ids is cut at 512 and the statistic counts the rest"""
    ix, v, L, alpha, ix2, st = I.dup_reference()
    assert st["dropped"] > 0
    with _engine(ix, ix.N + len(v)) as e:
        assert e.insert(v, L, alpha) == ix.N
        assert np.array_equal(e.entries(0, ix2.N), ix2.graph) and np.array_equal(e.codes(0, ix2.N), ix2.codes)
        s = e.insert_stats()
        assert (s["backedge_dropped"], s["backedge_appended"], s["backedge_pruned"]) == (st["dropped"], st["appended"], st["pruned"])


def test_a_wide_layout_is_refused():
    import stretch_inputs as S
    from bang_amd import BangError
    ix, _ = S.get("u8_48")                                                 # 8-bit, D / 16 = 3: outside bang_search_can_rerank
    with _engine(ix, ix.N + 16) as e:
        with pytest.raises(BangError, match="layout"):
            e.insert(ix.vectors()[:16], 32, 1.2)
        assert e.num_nodes() == ix.N


def test_two_batches_equal_the_reference_applied_twice():
    ix, v1, L, alpha = I.case("i8_a12")
    v2, ix2, _ = I.second_reference()
    _, _, L2, alpha2, _ = I.SECOND
    with _engine(ix, ix.N + len(v1) + len(v2)) as e:                       # (filled to the last node)
        assert e.insert(v1, L, alpha) == ix.N
        assert e.insert(v2, L2, alpha2) == ix.N + len(v1)
        assert np.array_equal(e.entries(0, ix2.N), ix2.graph) and np.array_equal(e.codes(0, ix2.N), ix2.codes)
        from bang_amd import BangError
        with pytest.raises(BangError, match="capacity"):
            e.insert(v2[:1], L2, alpha2)
        assert e.num_nodes() == ix2.N


@pytest.mark.parametrize("name", ["i8_a12", "u8_a12", "deep_a12", "f32_a12"])
def test_a_fresh_engine_on_the_export_answers_like_the_engine_that_inserted(name):
    ix, v, L, alpha = I.case(name)
    ix2, _ = I.reference(name)
    q = np.ascontiguousarray(np.concatenate([I.get(I.CASES[name][0])[1][:16], v[:16]]))
    ids_r, d_r, st_r = Reference(ix2).search(q, K, 48, "exact")
    found = np.unique(ids_r[(ids_r >= ix.N) & (ids_r < ix2.N)])
    assert len(found) >= 4, "the queries do not find the inserted points: nothing to exclude"
    with _engine(ix, ix.N + 128) as e:
        assert e.insert(v, L, alpha) == ix.N
        exported = e.export_index(ix)
        assert exported.N == ix2.N and np.array_equal(exported.graph, ix2.graph) and np.array_equal(exported.codes, ix2.codes)
        mine = {mode: _search(e, q, 48, mode) for mode in ("exact", "pq")}
        # an inserted id in the exclusion set is never returned; without the set it is
        hit = int(found[0])
        assert (mine["exact"][0] == hit).any()
        e.set_excluded([hit])
        for mode in ("exact", "pq"):
            assert not (_search(e, q, 48, mode)[0] == hit).any(), mode
        e.clear_excluded()
    with _engine(exported, None) as f:
        for mode in ("exact", "pq"):
            _same(_search(f, q, 48, mode), mine[mode], (name, mode))
    # ... and the exact walk is the CPU reference's on Index'
    _same(mine["exact"], (ids_r, _bits(d_r), st_r), (name, "reference"))


@pytest.mark.parametrize("name", ["u8", "f32"])
def test_capacity_alone_changes_no_result(name):
    ix, q = I.get(name)
    q = q[:24]
    with _engine(ix, None) as a, _engine(ix, ix.N + 1000) as b:
        for mode in ("exact", "pq"):
            _same(_search(b, q, 37, mode), _search(a, q, 37, mode), (name, mode))
        assert b.insert_stats()["capacity"] == ix.N + 1000 and a.insert_stats()["capacity"] == 0


def test_refusals():
    import bang_amd
    from bang_amd import BangError
    ix, v, L, alpha = I.case("deep_a12")
    # at load
    for opts in (dict(graph=bang_amd.GRAPH_HOST), dict(graph=bang_amd.GRAPH_AUTO), dict(graph=bang_amd.GRAPH_DEVICE, capacity=ix.N - 1)):
        with bang_amd.Engine(ix.dtype, **dict(dict(capacity=ix.N + 10), **opts)) as e:
            with pytest.raises(BangError, match="capacity"):
                e.load_index(ix)
            with pytest.raises(BangError, match="no index is loaded"):     # nothing was loaded: there are no nodes and no entries to touch
                e.num_nodes()
    # ... a caller's code buffer (it cannot grow) and vectors_fp16 = 1; the caller's buffer is left as it was
    from bang_amd import binding as B
    mine = B.DeviceBuffer.from_numpy(ix.codes, slack=256)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, capacity=ix.N + 10) as e:
        with pytest.raises(BangError, match="capacity.*code buffer"):
            e.load_index(ix, d_codes=mine.ptr)
        with pytest.raises(BangError, match="no index is loaded"):
            e.num_nodes()
        assert np.array_equal(mine.download(np.uint8, ix.codes.shape), ix.codes)
        e.load_index(ix)                                                   # the refused load left an engine that loads
        assert e.num_nodes() == ix.N and np.array_equal(e.entries(0, ix.N), ix.graph)
    mine.free()
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, capacity=ix.N + 10, vectors_fp16=1) as e:
        with pytest.raises(BangError, match="capacity.*vectors_fp16"):
            e.load_index(ix)
        with pytest.raises(BangError, match="no index is loaded"):
            e.num_nodes()
    # (a caller's VECTOR buffer reaches the engine through bang_load_stream_e / bang_load_shared_e only: tests/test_insert_abi.py)
    # no capacity: refused
    with _engine(ix, None) as e:
        with pytest.raises(BangError, match="capacity"):
            e.insert(v, L, alpha)
    with _engine(ix, ix.N + 70) as e:
        before = e.entries(0, ix.N)

        def refused(match, vec=v, L_=L, a=alpha):
            with pytest.raises(BangError, match=match):
                e.insert(vec, L_, a)
            assert e.num_nodes() == ix.N
        refused("capacity", np.concatenate([v, v[:7]]))                  # N + 71 > capacity
        refused("n = 0", v[:0])
        refused("n = 16385", np.zeros((16385, ix.D), np.float32))        # (checked in front of the capacity: no large index needed)
        refused("L_build", L_=0)
        refused("L_build", L_=513)
        for a in (float("nan"), float("inf"), 0.99, 8.5):
            refused("alpha", a=a)
        nanv = v.copy()
        nanv[5, 7] = np.nan
        refused("vector 5, dimension 7", nanv)
        e.set_labels(np.ones(ix.N, np.uint32))
        refused("label")
        e.clear_labels()
        e.set_searchparams(K, 40)
        e.alloc(8)
        refused("allocation")
        e.free()
        e.set_searchparams(K, 40, bang_amd.DIST_MIPS)
        refused("MIPS")
        e.set_searchparams(K, 40)
        assert np.array_equal(e.entries(0, ix.N), before), "a refused insert left a trace"
        assert e.insert(v, L, alpha) == ix.N                               # ... and the engine still inserts
        assert np.array_equal(e.entries(0, ix.N + len(v)), I.reference("deep_a12")[0].graph)
