"""The excluded ids (lazy deletes, DESIGN.md section 2 CANON 17) on the CPU: tests/exclude_reference.py composes the masked answer from what the
existing references return.  Pinned here, without a GPU: with X empty the composition IS each reference's own answer, bit for bit; hand-derived
answers on the toy inputs; and the masks tests/test_gpu_exclude.py uses reach the edges they are there for (counts asserted)."""
import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
import exclude_reference as X

K = 10
NQ = 32
PAD = int(X.PAD_ID)
BIG = np.float32(3.402823e38)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(_bits(got[1]), _bits(want[1]))


# ---------------------------------------------------------------------------------------------------------------------
# X empty: the composition is the references' own answer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (10, 37, 152))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_empty_set_reproduces_the_oracle(request, fixture, L):
    from oracle import oracle as O
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = q[:NQ]
    want = O.Oracle(ix).search(q, K, L, with_stats=True)
    ids, d, st, log, cnt = X.walk_base(ix, q, K, L)
    _same((ids, d), want)
    assert np.array_equal(st, want[2]) and np.array_equal(cnt, st[:, 1])
    _same(X.rerank_all(ix, q, log, cnt, [], K), want)
    if L == 37:                                                           # k = L
        _same(X.rerank_all(ix, q, log, cnt, [], L), O.Oracle(ix).search(q, L, L))


@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_empty_set_reproduces_every_reference(request, fixture):
    from oracle import oracle as O
    import exact_reference
    import beam_reference
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = q[:NQ]
    L = 37
    ids, d, st, log, cnt = X.walk_base(ix, q, K, L, layout="word")        # the word-local filter
    _same(X.rerank_all(ix, q, log, cnt, [], K), (ids, d))
    ids, d, st, log, cnt = X.walk_inmemory(ix, q, K, L)                   # semantics = 1
    _same(X.rerank_all(ix, q, log, cnt, [], K), (ids, d))
    assert log.shape[1] == L + 120
    if fixture == "small_f32":                                            # MIPS: the query one dimension short
        q1 = np.ascontiguousarray(q[:, :-1])
        want = O.Oracle(ix).search(q1, K, L, mips=True)
        ids, d, st, log, cnt = X.walk_base(ix, q1, K, L, mips=True)
        _same((ids, d), want)
        _same(X.rerank_all(ix, q1, log, cnt, [], K, mips=True), want)
    for beam in (1, 2):                                                   # distance = 1: first k of the worklist
        wl = X.walk_exact(ix, q, L, beam)
        want = exact_reference.Reference(ix).search(q, K, L, "exact") if beam == 1 else beam_reference.Reference(ix).search(q, K, L, beam)
        _same(X.worklist_all(wl[0], wl[1], [], K), want)
        _same(X.worklist_all(wl[0], wl[1], [], L), wl)
        assert np.array_equal(wl[2], want[2])                             # (k does not enter the walk)


# ---------------------------------------------------------------------------------------------------------------------
# hand-derived answers
# ---------------------------------------------------------------------------------------------------------------------
def _row(ids, dists=None):
    i = np.full(K, PAD, np.uint64)
    i[:len(ids)] = ids
    if dists is None:
        return i
    d = np.full(K, BIG, np.float32)
    d[:len(dists)] = dists
    return i, d


def test_shared_child_excluding_the_nearest_moves_every_later_result_up_one_rank():
    """0 -> {1, 2}; 1 -> {3, 4}; 2 -> {3, 5}; levels 100, 20, 30, 10, 15, 12; distance = 128 level^2.  Every node is expanded; by distance:
    3, 5, 4, 1, 2, 0.  Without node 3: 5, 4, 1, 2, 0 and five padding entries -- in the PQ walk and from the worklist of the exact walks."""
    ix, q = BI.shared_child()
    lv = {3: 10, 5: 12, 4: 15, 1: 20, 2: 30, 0: 100}
    full = [3, 5, 4, 1, 2, 0]
    ids, d, st, log, cnt = X.walk_base(ix, q, K, 10)
    assert sorted(log[0, :cnt[0]].tolist()) == [0, 1, 2, 3, 4, 5] and log[0, 0] == 0
    assert np.array_equal(ids[0], _row(full))
    for drop in ([3], [3, 3], np.array([3], np.uint32)):                  # (duplicates in the list are fine)
        gi, gd = X.masked_rerank(ix, q[0], log[0], cnt[0], drop, K)
        wi, wd = _row(full[1:], [128.0 * lv[x] ** 2 for x in full[1:]])
        assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd))
    for beam in (1, 2):
        wl = X.walk_exact(ix, q, 10, beam)
        assert np.array_equal(wl[0][0], _row(full))
        gi, gd = X.masked_worklist(wl[0][0], wl[1][:, 0], [3], K)
        wi, wd = _row(full[1:], [128.0 * lv[x] ** 2 for x in full[1:]])
        assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd))
        gi, _ = X.masked_worklist(wl[0][0], wl[1][:, 0], [3, 1, 0], 3)   # k live entries exactly: no padding
        assert gi.tolist() == [5, 4, 2]


def test_one_node_log_with_the_medoid_excluded_is_all_padding():
    ix, q = E.chain(n=1)                                                  # the medoid alone: nothing to walk to
    ids, d, st, log, cnt = X.walk_base(ix, q, K, 10)
    assert cnt[0] == 1 and log[0, 0] == ix.medoid and ids[0, 0] == ix.medoid and ids[0, 1] == PAD
    gi, gd = X.masked_rerank(ix, q[0], log[0], cnt[0], [int(ix.medoid)], K)
    assert np.array_equal(gi, _row([])) and np.array_equal(_bits(gd), _bits(np.full(K, BIG, np.float32)))


@pytest.mark.parametrize("L,entries", ((10, 60), (37, 87), (152, 202)))
def test_chain_fills_the_log_and_loses_what_is_excluded(L, entries):
    """i -> i + 1 with the distance falling: the walk runs to the iteration cap, the log is 0, 1, ... L + 49 -- one, two and four 64-entry
    pieces -- and the results are its last k nodes, nearest first.  Excluding the nearest moves the rest up; excluding log positions 0, 63, 64
    and the last leaves the others in order."""
    ix, q = E.chain()
    ids, d, st, log, cnt = X.walk_base(ix, q, K, L)
    assert cnt[0] == entries and log[0, :entries].tolist() == list(range(entries))
    assert ids[0].tolist() == list(range(entries - 1, entries - 1 - K, -1))
    gi, gd = X.masked_rerank(ix, q[0], log[0], cnt[0], [entries - 1], K)
    assert gi.tolist() == list(range(entries - 2, entries - 2 - K, -1)) and np.array_equal(_bits(gd[:K - 1]), _bits(d[1:, 0]))
    drop = [x for x in (0, 63, 64, entries - 1) if x < entries]
    gi, _ = X.masked_rerank(ix, q[0], log[0], cnt[0], drop, K)
    assert gi.tolist() == [x for x in range(entries - 1, -1, -1) if x not in drop][:K]
    gi, _ = X.masked_rerank(ix, q[0], log[0], cnt[0], list(range(5, 256)), K)          # five live candidates of sixty and more
    assert gi.tolist() == [4, 3, 2, 1, 0] + [PAD] * 5


def test_row_dup_loses_both_copies_of_node_2():
    """0 -> {1}; 1 -> {2, 2, 3}; 2 -> {4, 5}: the final worklist of the exact walks is 4, 5, 2, 2, 3, 1, 0."""
    ix, q = BI.row_dup()
    for beam in (1, 2):
        wl = X.walk_exact(ix, q, 10, beam)
        assert wl[0][0].tolist() == [4, 5, 2, 2, 3, 1, 0] + [PAD] * 3
        gi, gd = X.masked_worklist(wl[0][0], wl[1][:, 0], [2], K)
        assert gi.tolist() == [4, 5, 3, 1, 0] + [PAD] * 5
        assert np.array_equal(_bits(gd[:5]), _bits(wl[1][[0, 1, 4, 5, 6], 0])) and np.all(gd[5:] == BIG)
        gi, _ = X.masked_worklist(wl[0][0], wl[1][:, 0], [4], 3)           # ... and each is kept where it is not excluded
        assert gi.tolist() == [5, 2, 2]


# ---------------------------------------------------------------------------------------------------------------------
# the masks of the GPU file reach their edges on the reference
# ---------------------------------------------------------------------------------------------------------------------
def _edge_counts(ix, q, L):
    ids, d, st, log, cnt = X.walk_base(ix, q, K, L)
    out = {}
    for name in X.MASKS:
        m = X.as_set(X.make_mask(name, ix, ids[:, 0]))
        short = hit0 = hit63 = hit64 = hitlast = allgone = 0
        for i in range(q.shape[0]):
            lg = log[i, :cnt[i]].tolist()
            short += sum(x not in m for x in lg) < K
            hit0 += lg[0] in m
            hit63 += len(lg) > 63 and lg[63] in m
            hit64 += len(lg) > 64 and lg[64] in m
            hitlast += lg[-1] in m
            allgone += all(int(x) in m for x in ids[i] if int(x) != PAD)
        out[name] = (short, hit0, hit63, hit64, hitlast, allgone)
    return out


def test_masks_reach_their_edges_on_small_u8(small_u8):
    """Per mask, over the 32 queries at L = 152 (logs of 153 .. 156 entries: three pieces): queries left with fewer than k live candidates;
    queries with an excluded id at log position 0, 63, 64, and the last; queries whose unmasked results are all excluded."""
    ix, q, _, _ = small_u8
    c = _edge_counts(ix, q[:NQ], 152)
    assert c["all_but_one"][0] == NQ and c["all_but_one"][5] >= NQ - 1     # fewer than k left; every unmasked result gone
    assert c["edges"][1] == NQ and c["all_but_one"][1] >= NQ - 1           # position 0 is the medoid
    for name in ("rand30", "all_but_one"):
        assert min(c[name][2:5]) >= 1, (name, c[name])                     # positions 63, 64 and the last
    assert c["top"][0] == 0 and all(v[0] == 0 for k_, v in c.items() if k_ != "all_but_one")
    assert c == EDGE_COUNTS_U8_152, c


def test_masks_reach_their_edges_on_the_chain():
    """One query, a log of exactly L + 50 entries: `edges` excludes positions 0, 31, 32 and the last node of the index; all_but_one leaves at most one."""
    ix, q = E.chain()
    for L, entries in ((10, 60), (37, 87), (152, 202)):
        ids, d, st, log, cnt = X.walk_base(ix, q, K, L)
        m = X.as_set(X.make_mask("all_but_one", ix))
        live = [x for x in log[0, :cnt[0]].tolist() if x not in m]
        assert cnt[0] == entries and len(live) <= 1
        gi, _ = X.masked_rerank(ix, q[0], log[0], cnt[0], sorted(m), K)
        assert gi.tolist() == live + [PAD] * (K - len(live))
        top = X.make_mask("top", ix, ids[:, 0])
        assert top.tolist() == [entries - 1]


# (short, position 0, position 63, position 64, last position, every unmasked result excluded) per mask: small_u8, 32 queries, k = 10, L = 152
EDGE_COUNTS_U8_152 = {"rand30": (0, 0, 9, 8, 10, 0), "top": (0, 0, 0, 1, 1, 0), "edges": (0, 32, 0, 0, 0, 0), "all_but_one": (32, 32, 32, 32, 32, 32)}
