"""Inserts on a GPU (csrc/bang_insert.hip, bang_insert_e), bit for bit against tests/insert_reference.py: bang_k_prune on lists of 0 .. 512
entries, at every vector layout, at the edges of its kill rule (lattice points: alpha2 * e == d_t, the float32 rounding of the product), at R = 1
and 5, with count words beyond the stride and beyond 512, and into a copy of the graph table; bang_k_backedge at every layout and on its edge
targets; bang_k_pq_encode on the four pivot layouts and at m = 1 .. 129 with ties; and the engine -- entries and codes after one and two batches,
with the three chunk seams crossed (test hooks BANG_INSERT_*_CHUNK), an engine loaded from the export against the engine that inserted in
every search form, an excluded inserted id, and the refusals."""
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
    return I.make_list(ref, rng, node, length, pool)


def _prune_gpu(ix, lists, owns, R, alpha, graph_ptr=None, entry_len=None, n_nodes=None, max_wgs=0, max_waves=0, stride=None, cnt_words=None):
    """-> (rows u32 [n_lists][R + 1], abort word); cnt_words: the count words as the kernel reads them (default: the lists' lengths)"""
    from bang_amd import binding as B
    n = len(lists)
    stride = stride or max(1, max(len(l[0]) for l in lists))
    ids = np.zeros((n, stride), np.uint32)
    d = np.zeros((n, stride), np.float32)
    cnt = np.zeros(n, np.uint32)
    for i, (a, b) in enumerate(lists):
        ids[i, :len(a)], d[i, :len(a)], cnt[i] = a, b, len(a)
    if cnt_words is not None:
        cnt[:] = cnt_words
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


def _nineteen_lists(ref, R, alpha):
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
    return lists, owns


@pytest.mark.parametrize("alpha", [1.2, 8.0])
@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("name", ["i8", "u8", "deep", "f32"])
def test_prune_every_length(name, R, alpha):
    """lists of 0, 1, 63, 64, 65 and 512 entries, three of each, one with its own id inside; 8 waves in 4 workgroups of two take 19 lists:
    every wave takes a second list and the last round leaves workgroups partly idle"""
    ref = _ref(name)
    ix = ref.ix
    lists, owns = _nineteen_lists(ref, R, alpha)
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


@pytest.mark.parametrize("name", sorted(I.LAYOUTS))
def test_prune_every_layout(name):
    """the picked candidate's vector as the wave's query at the layouts the four indexes leave out: G = 1, 2 and 16 pieces (8-bit D = 16, 32, 256),
    float D = 4, D = 160 (a partly filled third register), D = 200 (a partly filled fourth) and D = 256 (four full registers); lists of 1, 64, 65 and 200 entries"""
    ix = I.layout(name)
    ref = Reference(ix)
    rng = np.random.default_rng(ix.D)
    owns = [int(t) for t in rng.integers(ix.N, size=4)]
    lists = [_make_list(ref, rng, t, n) for t, n in zip(owns, (1, 64, 65, 200))]
    want = _want_rows(ref, lists, owns, ix.R, 1.2)
    assert (want[1:, 0] >= 2).all(), "a list with one pick computes no distance"
    got, abort = _prune_gpu(ix, lists, owns, ix.R, 1.2, max_wgs=2, max_waves=2)
    assert abort == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("kind", sorted(I.LATTICES))
@pytest.mark.parametrize("iname", ["i8", "u8"])
def test_prune_kill_rule_on_lattice_points(iname, kind, alpha):
    """integer lattice points: at alpha = 1 kills are decided at alpha2 * e == d_t ('<=', not '<'), at alpha = 1.2 by the float32 rounding of the one
    multiply (tests/test_insert_reference.py shows on the CPU that a rule with '<', or with an unrounded product, gives other rows)"""
    ix = I.lattice(iname, kind)
    ref = Reference(ix)
    lists, owns = I.lattice_lists(iname, kind)
    want = _want_rows(ref, lists, owns, ix.R, alpha)
    got, abort = _prune_gpu(ix, lists, owns, ix.R, alpha, max_wgs=2, max_waves=2)
    assert abort == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("R", [1, 5])
def test_prune_rows_of_one_and_of_five_ids(R):
    """R = 1: the row is full at the first pick; R = 5: an odd row, 6 of 64 lanes store it"""
    ref = _ref("i8")
    lists, owns = _nineteen_lists(ref, R, 1.2)
    want = _want_rows(ref, lists, owns, R, 1.2)
    assert (want[:, 0] == R).any() and (want[:, 0] == 0).any()
    got, abort = _prune_gpu(ref.ix, lists, owns, R, 1.2, max_wgs=4, max_waves=2)
    assert abort == 0 and np.array_equal(got, want)


def test_prune_count_words_beyond_the_stride_and_beyond_512():
    """a count word of stride + 9 reads `stride` entries (behind them lie the next list's, which would change the row); 600 entries at a stride of
    600 are cut at 512 (the entries behind would change the row)"""
    ref = _ref("i8")
    ix = ref.ix
    rng = np.random.default_rng(21)
    lists = [_make_list(ref, rng, 40, 70), _make_list(ref, rng, 41, 70)]
    owns = [40, 41]
    want = _want_rows(ref, lists, owns, ix.R, 1.2)
    over = (np.concatenate([lists[0][0], lists[1][0][:9]]), np.concatenate([lists[0][1], lists[1][1][:9]]))
    assert not np.array_equal(_want_rows(ref, [over], owns[:1], ix.R, 1.2)[0], want[0]), "the nine entries behind the stride would not show"
    got, abort = _prune_gpu(ix, lists, owns, ix.R, 1.2, stride=70, cnt_words=[79, 70])
    assert abort == 0 and np.array_equal(got, want)
    # 600 entries in order: the nearest id 501 times (the copies die at e = 0), 11 more in front of entry 512 and 88 behind it
    long = []
    for node in (42, 43):
        a, b = _make_list(ref, rng, node, 100)
        rep = np.concatenate([np.zeros(501, np.int64), np.arange(1, 100)])
        long.append((a[rep], b[rep]))
        assert len(long[-1][0]) == 600
    cut = [(a[:512], b[:512]) for a, b in long]
    want = _want_rows(ref, cut, [42, 43], ix.R, 1.2)
    assert not np.array_equal(_want_rows(ref, long, [42, 43], ix.R, 1.2), want), "the entries behind 512 would not show"
    got, abort = _prune_gpu(ix, long, [42, 43], ix.R, 1.2, stride=600, cnt_words=[600, 600])
    assert abort == 0 and np.array_equal(got, want)


def test_prune_into_the_graph_table_changes_the_named_rows_only():
    """the engine's call shape: out_by_own = 1, d_out = graph + vec_bytes, out_stride = entry_len -- between two rows lie other nodes' vectors; a
    tenth list with own = n_nodes sets the abort word and leaves the (marked) entry behind the table alone"""
    from bang_amd import binding as B
    ref = _ref("u8")
    ix = ref.ix
    vb, R = ix.D, ix.R
    rng = np.random.default_rng(8)
    owns = [int(x) for x in rng.choice(ix.N, 9, replace=False)] + [ix.N]  # nine rows of the table; the tenth lies behind it
    lists = [_make_list(ref, rng, t if t < ix.N else 0, n) for t, n in zip(owns, (0, 1, 40, 64, 65, 100, 130, 200, 512, 80))]
    n = len(lists)
    stride = 512
    ids, d, cnt = np.zeros((n, stride), np.uint32), np.zeros((n, stride), np.float32), np.zeros(n, np.uint32)
    for i, (a, b) in enumerate(lists):
        ids[i, :len(a)], d[i, :len(a)], cnt[i] = a, b, len(a)
    # the table with two marked spare entries behind node N - 1: a row written for own = N would land in the first of them
    table = np.concatenate([ix.graph, np.full((2, ix.entry_len), 0xA5, np.uint8)])
    g = B.DeviceBuffer.from_numpy(table, slack=256)
    bufs = [B.DeviceBuffer.from_numpy(x) for x in (ids, d, cnt, np.asarray(owns, np.uint32))]
    ab = B.DeviceBuffer(4)
    p = B.PruneParams()
    p.d_graph, p.entry_len, p.dtype, p.D, p.n_nodes, p.R = g.ptr, ix.entry_len, B.DTYPE_CODE[ix.dtype], ix.D, ix.N, R
    p.alpha2, p.n_lists, p.list_stride = float(IR.alpha2_of(1.2)), n, stride
    p.d_list_ids, p.d_list_dists, p.d_list_cnt, p.d_own = (b.ptr for b in bufs)
    p.d_out, p.out_stride, p.out_by_own, p.max_wgs, p.max_waves, p.d_abort = g.ptr + vb, ix.entry_len, 1, 2, 2, ab.ptr
    fn = B.lib().bang_k_prune
    fn.argtypes = [C.c_void_p, C.c_void_p]
    B._check(fn(C.byref(p), None), "bang_k_prune")
    B.sync()
    after, abort = g.download(np.uint8, table.shape), int(ab.download(np.uint32, (1,))[0])
    for b in bufs + [g, ab]:
        b.free()
    want = table.copy()
    want[owns[:9], vb:] = _want_rows(ref, lists[:9], owns[:9], R, 1.2).view(np.uint8)
    assert abort == 2, "a row outside the table was not reported"
    assert (after[ix.N:] == 0xA5).all(), "the list whose own node lies behind the table wrote a row"
    assert np.array_equal(after, want), "the nine rows, and no other byte of the table"
    assert not np.array_equal(after[:ix.N], ix.graph)


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


@pytest.mark.parametrize("name", sorted(I.LAYOUTS))
def test_backedge_every_layout(name):
    """the target's vector as the wave's query at every layout: one target that appends, one whose candidates (old row ++ new ids) get their exact
    distances"""
    from bang_amd import formats
    ix = I.layout(name)
    R, N, vb = ix.R, ix.N, ix.D * (4 if ix.dtype == "float" else 1)
    new = I.batch(ix, 16, 3)
    graph = np.concatenate([ix.graph, formats.pack_graph(new, np.zeros(16, np.uint32), np.zeros((16, R), np.uint32))])
    rows = graph[:, vb:].view(np.uint32)
    t0, t1 = (int(x) for x in np.flatnonzero(rows[:N, 0] == R)[:2])
    rows[t0, 0] = R - 2
    rows[t0, 1 + R - 2:] = 0
    before = graph.copy()
    inc = [np.array([N + 3, N + 11]), np.array([N, N + 7, N + 15])]
    ref = Reference(dataclasses.replace(ix, N=N + 16, graph=before, codes=np.zeros((N + 16, ix.m), np.uint8)))
    after, ci, cd, offered, own, stats, abort = _backedge_gpu(ix, before, N + 16, [t0, t1], inc)
    want = before.copy()
    wrows = want[:, vb:].view(np.uint32)
    wrows[t0, 1 + R - 2: 1 + R] = inc[0]
    wrows[t0, 0] = R
    assert abort == 0 and stats == [1, 1, 0] and np.array_equal(after, want)
    cand = np.concatenate([before[t1, vb:].view(np.uint32)[1:1 + R], inc[1]]).astype(np.uint32)
    assert list(offered) == [0, R + 3] and list(own) == [0xFFFFFFFF, t1]
    assert np.array_equal(ci[1, :R + 3], cand) and np.array_equal(cd[1, :R + 3], _bits(ref.exact(cand, IR.vector_of(ref, t1))))
    assert (ci[0] == 0xCDCDCDCD).all() and (ci[1, R + 3:] == 0xCDCDCDCD).all() and (cd[1, R + 3:] == 0xCDCDCDCD).all()


@pytest.mark.parametrize("name", ["i8", "u8", "f32"])
def test_backedge_edges(name):
    """seven targets per launch (the last workgroup runs 3 of its 4 waves): no incoming id; an empty row that takes R ids; a row of one id that
    overflows with R + 1 candidates; 130 incoming ids (three 64-lane pieces of the source part); a row word of R + 7 (read as R); 64 + 500 candidates
    (cut at 512, 52 dropped); an id outside the index at source position 0, or -- second launch -- at candidate 64, the start of a piece"""
    from bang_amd import formats
    ix, _ = I.get(name)
    R, N, vb = ix.R, ix.N, ix.D * (4 if ix.dtype == "float" else 1)
    NEW, SKIP, MARK = 600, 0xFFFFFFFF, 0xCDCDCDCD
    new = I.batch(ix, NEW, 9)
    graph = np.concatenate([ix.graph, formats.pack_graph(new, np.zeros(NEW, np.uint32), np.zeros((NEW, R), np.uint32))])
    rows = graph[:, vb:].view(np.uint32)
    t = [int(x) for x in np.flatnonzero(rows[:N, 0] == R)[:8]]
    assert len(t) == 8
    rows[t[1], :] = 0                                                      # an empty row
    rows[t[2], 0] = 1
    rows[t[2], 2:] = 0
    rows[t[4], 0] = R + 7                                                  # a corrupt degree word over a sound row
    deg_b = min(R, 40)                                                     # the last target: the bad id becomes candidate 64
    rows[t[7], 0] = deg_b
    rows[t[7], 1 + deg_b:] = 0
    before = graph.copy()
    bad = N + NEW + 5
    ids = lambda k, first=0: (N + first + np.arange(k)).astype(np.uint32)  # noqa: E731
    inc = [ids(0), ids(R, 7), ids(R, 100), ids(130, 50), ids(3, 590), ids(64 + 500 - R), np.concatenate([[bad], ids(2, 20)]).astype(np.uint32),
           np.concatenate([ids(64 - deg_b, 300), [bad], ids(5, 400)]).astype(np.uint32)]
    deg = [R, 0, 1, R, R, R, R, deg_b]                                     # as the kernel reads them
    assert all(deg[i] + len(inc[i]) > R for i in (2, 3, 4, 5, 6, 7)) and deg[1] + len(inc[1]) == R and deg[7] + len(inc[7]) > 64
    ref = Reference(dataclasses.replace(ix, N=N + NEW, graph=before, codes=np.zeros((N + NEW, ix.m), np.uint8)))
    for launch in ([0, 1, 2, 3, 4, 5, 6], [7, 0, 1, 2, 3, 4, 5]):
        after, ci, cd, offered, own, stats, abort = _backedge_gpu(ix, before, N + NEW, [t[i] for i in launch], [inc[i] for i in launch])
        assert abort == 2
        want = before.copy()
        wrows = want[:, vb:].view(np.uint32)
        wrows[t[1], 0] = R
        wrows[t[1], 1:] = inc[1]
        assert np.array_equal(after, want), "the row that appended R ids, and no other byte of the table (a target without incoming ids keeps its row)"
        for slot, i in enumerate(launch):
            if i in (0, 1):                                                # appended
                assert offered[slot] == 0 and own[slot] == SKIP and (ci[slot] == MARK).all() and (cd[slot] == MARK).all(), i
                continue
            cand = np.concatenate([before[t[i], vb:].view(np.uint32)[1:1 + deg[i]], inc[i]]).astype(np.uint32)[:512]
            if (cand == bad).any():
                cand = cand[:int(np.argmax(cand == bad))]                  # the list ends in front of the id
            n = len(cand)
            assert n == {2: R + 1, 3: R + 130, 4: R + 3, 5: 512, 6: R, 7: 64}[i]
            assert offered[slot] == n and own[slot] == t[i], i
            assert np.array_equal(ci[slot, :n], cand) and np.array_equal(cd[slot, :n], _bits(ref.exact(cand, IR.vector_of(ref, t[i])))), i
            assert (ci[slot, n:] == MARK).all() and (cd[slot, n:] == MARK).all(), i
        assert stats == [2, 5, 52]


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


@pytest.mark.parametrize("name", sorted(I.PQ_LAYOUTS))
def test_pq_encode_chunk_passes_and_ties(name):
    """m = 1, 64, 65, 128, 129: one to three passes of 64 chunks with tails of 0 and 1; equal pivot rows k and k + 64 (one lane's strict '<'), 70 and
    133 (the lower k in the higher lane: the second word of the wave's minimum), 0 and 255; 9 vectors in chunks of 4 tables"""
    ix, v = I.pq_layout(name)
    ref = Reference(ix)
    want = np.stack([IR.encode(ref, x) for x in v])
    assert all((want == lo).any() for lo, _ in I.PQ_TIES)
    for stride in (ix.m, ix.m + 3):
        got = _encode_gpu(ix, v, 4, stride)
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


@pytest.mark.parametrize("name", sorted(I.SEAMS))
def test_chunk_seams_change_nothing(name, monkeypatch):
    """the search + prune, back-edge and encode steps in small chunks (test hooks): the reference knows no chunks, so entries, codes and statistics
    are its own.  tests/test_insert_reference.py shows that every seam is crossed with data that differ from the first chunk's"""
    ix, v, L, alpha, ix2, st = I.seam_case(name)
    for var, val in zip(("BANG_INSERT_SEARCH_CHUNK", "BANG_INSERT_TARGET_CHUNK", "BANG_INSERT_ENCODE_CHUNK"), I.SEAMS[name]):
        monkeypatch.setenv(var, str(val))
    with _engine(ix, ix.N + len(v) + 3) as e:
        assert e.insert(v, L, alpha) == ix.N
        entries, codes, s = e.entries(0, ix2.N), e.codes(0, ix2.N), e.insert_stats()
    assert np.array_equal(entries, ix2.graph)
    assert np.array_equal(codes, ix2.codes)
    assert s == dict(capacity=ix.N + len(v) + 3, inserted=st["inserted"], backedge_appended=st["appended"], backedge_pruned=st["pruned"],
                     backedge_dropped=st["dropped"])


def test_chunk_hooks_are_clamped(monkeypatch):
    """the lower clamp: 0 and a negative value are taken as 1 (a chunk of 0 would never end).  A value above the engine's own size is merely
    accepted here: with 16 points the upper clamp cannot show in a result"""
    ix, v, L, alpha = I.case("i8_a8")
    ix2, st = I.reference("i8_a8")
    for vals in (("0", "-5", "0"), ("100000", "100000", "100000")):
        for var, val in zip(("BANG_INSERT_SEARCH_CHUNK", "BANG_INSERT_TARGET_CHUNK", "BANG_INSERT_ENCODE_CHUNK"), vals):
            monkeypatch.setenv(var, val)
        with _engine(ix, ix.N + len(v)) as e:
            assert e.insert(v, L, alpha) == ix.N
            assert np.array_equal(e.entries(0, ix2.N), ix2.graph) and np.array_equal(e.codes(0, ix2.N), ix2.codes), vals
            assert e.insert_stats()["backedge_pruned"] == st["pruned"]


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


# ---------------------------------------------------------------------------------------------------------------------
# every search form the engine offers with the graph in HBM, on an engine that inserted
# ---------------------------------------------------------------------------------------------------------------------
FORM_L = 48
# form -> (options for bang_load, options for bang_alloc, the cases it runs on)
_WALK = ("i8_a12", "f32_a12")
FORMS = {
    "search0":        ({}, dict(distance=0, search=0), _WALK),
    "search1":        ({}, dict(distance=0, search=1, fuse_rerank=1), _WALK),
    "fuse_rerank0":   ({}, dict(distance=0, search=1, fuse_rerank=0), _WALK),
    "semantics1":     ({}, dict(distance=0, search=1, semantics=1), _WALK),
    "filter_layout1": ({}, dict(distance=0, search=1, filter_layout=1), _WALK),
    "beam2":          ({}, dict(distance=1, search=1, beam=2), _WALK),
    "beam4":          ({}, dict(distance=1, search=1, beam=4), _WALK),
    "range":          ({}, dict(distance=1, search=1, range_hits=512), _WALK),
    "labels":         ({}, dict(distance=1, search=1), _WALK),
    "pq1":            (dict(pq=1), dict(distance=0, search=1), I.FORM_CASES),
    "code_stride0":   (dict(code_stride=0), dict(distance=0, search=1), I.FORM_CASES),
    "pq_ragged0":     (dict(pq_ragged=0), dict(distance=0, search=1), I.FORM_CASES),     # (no counter tells the padded pivot table from the exact-size
}                                                                                        #  one, and the answers are the same by design)


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _form_reference(form, name, ix2, q):
    """what the CPU reference of the form answers on Index': a dict of the arrays _form_run returns (a subset: what the reference defines)"""
    if form in ("search0", "search1", "fuse_rerank0", "pq1", "code_stride0", "pq_ragged0"):
        from oracle import oracle as O
        ids, d, st = _cached(("oracle", name), lambda: O.Oracle(ix2).search(q, K, FORM_L, with_stats=True))
        out = dict(ids=ids, d=_bits(d))
        if form != "search0":                                              # (the per-iteration kernels keep no per-query counters)
            out["counters"] = st
        return out
    # semantics and beam have no counter in bang_get_stats: that the option took effect shows in the reference's answer, which must therefore
    # differ from the plain walk's (asserted here) -- an engine that ignored the option would give the plain walk's counters
    if form == "semantics1":
        import inmemory_reference
        from oracle import oracle as O
        ids, d, st = inmemory_reference.Reference(ix2).search(q, K, FORM_L, "inmemory")
        plain = _cached(("oracle", name), lambda: O.Oracle(ix2).search(q, K, FORM_L, with_stats=True))
        assert not np.array_equal(st, plain[2]), "the Inmemory walk's counters equal BANG_Base's on these queries"
        return dict(ids=ids, d=_bits(d), counters=st)
    if form == "filter_layout1":
        import wordfilter_reference
        ids, d, st = wordfilter_reference.Reference(ix2).search(q, K, FORM_L, "word")
        return dict(ids=ids, d=_bits(d), counters=st)
    if form in ("beam2", "beam4"):
        import beam_reference
        ids, d, st, _ = beam_reference.Reference(ix2).search(q, K, FORM_L, int(form[4:]))
        plain = _cached(("exact", name), lambda: Reference(ix2).search(q, K, FORM_L, "exact"))
        assert not np.array_equal(st, plain[2]), "the beam walk's counters equal the one-parent walk's on these queries"
        return dict(ids=ids, d=_bits(d), counters=st)
    if form == "range":
        import range_reference as RR
        ref = _cached(("range ref", name), lambda: RR.Reference(ix2))
        tr = ref.evaluated_all(q, FORM_L)
        top_ids, top_d, top_st = _cached(("exact", name), lambda: Reference(ix2).search(q, K, FORM_L, "exact"))   # the same walk's k results
        out = {}
        for rname, r in _form_radii(name, ix2, q):
            lims, ids, d, counts, offered = RR.collect_all(tr, r, 512)
            out[rname] = dict(ids=top_ids, d=_bits(top_d), lims=lims, hit_ids=ids, hit_d=_bits(d), counts=counts, offered=offered,
                              counters=np.array([t.stats for t in tr], np.int64))
            assert np.array_equal(out[rname]["counters"], top_st)
        return out
    if form == "labels":
        import labels_inputs as LI
        import labels_reference as LR
        any_, all_ = LI.batch("mixed", q.shape[0])
        ids, d, matched, st, _ = LR.collect_all(LR.Reference(ix2).walks(q, FORM_L), LI.rand4(ix2.N), any_, all_, K, FORM_L, int(ix2.medoid))
        return dict(ids=ids, d=_bits(d), matched=matched, counters=st)
    raise ValueError(form)


def _form_radii(name, ix2, q):
    import range_inputs as RI
    import range_reference as RR
    ref = _cached(("range ref", name), lambda: RR.Reference(ix2))
    return [(r, RI.radii(r, ref, ix2, q)) for r in ("rank100", "mixed")]


def _form_run(e, form, alloc_opts, name, ix2, q):
    """one batch (two for the range form: one per set of radii) on a loaded, unallocated engine -> dict of arrays"""
    Q = q.shape[0]
    for key, val in alloc_opts.items():
        e.set_option(key, val)
    e.set_searchparams(K, FORM_L)
    if form == "labels":
        import labels_inputs as LI
        e.set_labels(LI.rand4(ix2.N))
    e.alloc(Q)
    if form == "range":
        out = {}
        for rname, r in _form_radii(name, ix2, q):
            e.set_radii(r)
            e.init(Q)
            ids, d = e.query(q)
            counts, offered = e.range_counts(Q)
            lims, hit_ids, hit_d = e.range_results(Q)
            out[rname] = dict(ids=ids, d=_bits(d), counters=e.query_counters(Q), counts=counts, offered=offered, lims=lims, hit_ids=hit_ids,
                              hit_d=_bits(hit_d))
            st = e.stats()
            assert st["search_kernel"] == 1 and st["range_launches"] == 1 and st["range_queries"] == Q and st["range_hits"] == 512, (form, st)
        e.free()
        return out
    if form == "labels":
        e.set_filters(*LI.batch("mixed", Q))
    e.init(Q)
    ids, d = e.query(q)
    out = dict(ids=ids, d=_bits(d), counters=e.query_counters(Q))
    if form == "labels":
        out["matched"] = e.matched_counts(Q)
    # the engine ran the form that was asked for
    st = e.stats()
    assert st["search_kernel"] == (0 if form == "search0" else 1) and st["front_launches"] >= 1, (form, st)
    if form in ("fuse_rerank0", "pq1"):                                    # (the LUT-path kernel never fuses the re-rank; the LDS-table kernel does,
        assert st["rerank_fused"] == 0, st                                 #  which is how pq = 1 shows in the counters)
    if form in ("search1", "code_stride0"):
        assert st["rerank_fused"] == 1, st
    if form == "filter_layout1":
        assert st["filter_layout"] == 1, st
    if form == "labels":
        assert st["label_launches"] == 1 and st["labelled"] == ix2.N and st["filtered_queries"] == 16, st
    if form == "code_stride0":
        assert st["code_stride"] == ix2.m, st
    e.free()
    return out


def _same_dicts(got, want, what, subset=False):
    """every array of `want` equals that of `got`; unless subset, they hold the same arrays"""
    assert subset or sorted(got) == sorted(want), what
    for key, w in want.items():
        if isinstance(w, dict):
            _same_dicts(got[key], w, what + (key,), subset)
        else:
            assert np.array_equal(got[key], w), what + (key,)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_after_an_insert(form):
    """engine A loads with capacity and inserts; engine B is fresh on A's export.  24 queries (16 of the index's, 8 inserted vectors; k = 10,
    L = 48) give the same results and counters on both -- and what the form's CPU reference answers on Index', for equality of two engines
    that share a defect proves nothing.  Under the load-time variants the insert itself still equals the reference byte for byte."""
    load_opts, alloc_opts, cases = FORMS[form]
    for name in cases:
        ix, v, L, alpha = I.case(name)
        ix2, _ = I.reference(name)
        q = I.form_queries(name)
        with _engine(ix, ix.N + 128, **load_opts) as a:
            assert a.insert(v, L, alpha) == ix.N
            assert np.array_equal(a.entries(0, ix2.N), ix2.graph) and np.array_equal(a.codes(0, ix2.N), ix2.codes), (form, name)
            exported = a.export_index(ix)
            mine = _form_run(a, form, alloc_opts, name, ix2, q)
        with _engine(exported, None, **load_opts) as b:
            _same_dicts(_form_run(b, form, alloc_opts, name, ix2, q), mine, (form, name, "fresh engine"))
        _same_dicts(mine, _form_reference(form, name, ix2, q), (form, name, "reference"), subset=True)
        found = np.unique(np.concatenate([x["ids"] for x in (mine.values() if form == "range" else [mine])]))
        assert ((found >= ix.N) & (found < ix2.N)).sum() >= 4, (form, name, "the answers hold fewer than 4 inserted ids")
