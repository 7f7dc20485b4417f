"""Per-query label filters on the exact-distance walk (CANON 18), without a GPU: the CPU reference of tests/labels_reference.py
against exact_reference (an unfiltered query is today's answer, bit for bit), hand-derived answers on the toy inputs, and the edge counts the GPU
inputs of tests/test_gpu_labels.py must reach."""
import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
import exact_reference as XR
import labels_inputs as LI
import labels_reference as LR

NQ = 32
K = 10
LS = (10, 37, 152)
PAD = int(LR.PAD_ID)
_CACHE = {}


def _traces(name, ix, q, L):
    key = (name, q.shape, L)
    if key not in _CACHE:
        _CACHE[key] = LR.Reference(ix).walks(q, L)
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ids(res):
    return [int(x) for x in res[0] if int(x) != PAD]


@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
@pytest.mark.parametrize("L", LS)
def test_an_unfiltered_query_is_the_exact_reference_bit_for_bit(request, fixture, L):
    """any = all = 0 on a random table: the result list of capacity L, fed the survivors of every merged iteration through the worklist's own rule,
    ends as the worklist does.  Counters and the final worklist of the trace are exact_reference's as well."""
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = np.ascontiguousarray(q[:NQ])
    tr = _traces(fixture, ix, q, L)
    ids_x, d_x, st_x = XR.Reference(ix).search(q, K, L, "exact")
    zero = np.zeros(NQ, np.uint32)
    ids, d, matched, st, _ = LR.collect_all(tr, LI.rand4(ix.N), zero, zero, K, L, int(ix.medoid))
    assert np.array_equal(ids, ids_x) and np.array_equal(_bits(d), _bits(d_x)) and np.array_equal(st, st_x)
    ids_L, d_L, _, _, _ = LR.collect_all(tr, LI.rand4(ix.N), zero, zero, L, L, int(ix.medoid))
    for i, t in enumerate(tr):
        n = len(t.wl_ids)
        assert np.array_equal(ids_L[i, :n], t.wl_ids.astype(np.uint64)) and np.array_equal(_bits(d_L[:n, i]), _bits(t.wl_dists))
        assert matched[i] == sum(len(S) for _, S, _ in t.merged)


# ---------------------------------------------------------------------------------------------------------------------
# hand-derived answers
# ---------------------------------------------------------------------------------------------------------------------
def _one(ix, q, L, labels, any_=1, all_=0, k=K, excluded=None):
    t = LR.Reference(ix).walk(q[0], L)
    return LR.collect(t, labels, any_, all_, k, L, int(ix.medoid), excluded), t


def test_chain_every_third_node():
    """0 -> 1 -> ... -> 255, distance falling: at L = 10 the walk stops at the cap, iteration 59, whose survivor (node 59) is not merged.  The merged
    survivors are the nodes 0 .. 58; those divisible by 3, nearest first, are 57, 54, ..., 30 -- ten of them.  The final worklist holds 58 .. 49, of
    which only 57, 54, 51 match."""
    ix, q = E.chain()
    labels = np.where(np.arange(ix.N) % 3 == 0, 1, 0).astype(np.uint32)
    res, t = _one(ix, q, 10, labels)
    assert _ids(res) == list(range(57, 29, -3))
    assert res[2] == 20 and res[3] == 1                          # 0, 3, ..., 57 offered; the medoid (node 0) in the first iteration
    assert [int(x) for x in t.wl_ids] == list(range(58, 48, -1))
    assert _ids(LR.worklist_pick(t, labels, 1, 0, K)) == [57, 54, 51]


def test_row_dup_puts_the_id_in_twice():
    """0 -> {1}; 1 -> {2, 2, 3}: both copies of node 2 pass the filter (the state at the iteration's entry) and both enter, as in the worklist."""
    ix, q = BI.row_dup()
    labels = np.zeros(ix.N, np.uint32)
    labels[2] = 1
    res, _ = _one(ix, q, 10, labels)
    assert _ids(res) == [2, 2] and res[2] == 2
    assert np.array_equal(_bits(res[1][:2]), _bits(res[1][:1].repeat(2)))


@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed65_the_sixty_fifth_survivor(variant):
    """The seed list [medoid, 1 .. 64] has 65 survivors.  Only node 64 matching: the result is [64], whatever lane-less element 64's rank.  All
    matching: the unfiltered answer, and 75 of the 76 nodes are offered (node 71, behind node 1, is never reached)."""
    ix, q = E.seed65("uint8", variant)
    labels = np.zeros(ix.N, np.uint32)
    labels[64] = 1
    res, t = _one(ix, q, 10, labels)
    assert _ids(res) == [64] and res[2] == 1 and res[3] == 1
    every = np.ones(ix.N, np.uint32)
    res, t = _one(ix, q, 10, every)
    want = XR.Reference(ix).search_one(q[0], K, 10, "exact")
    assert np.array_equal(res[0], want[0]) and np.array_equal(_bits(res[1]), _bits(want[1]))
    assert res[2] == 75 and res[4][0] == 65
    labels = every.copy()
    labels[5] = 0
    res, _ = _one(ix, q, 10, labels)
    assert res[4][0] == 64 and res[2] == 74


def test_short_worklist_without_node_1():
    """Three nodes at levels 30, 10, 20: the worklist ends as [1, 2, 0]; without node 1 the results are [2, 0] and eight padded entries."""
    ix, q = E.short_worklist()
    labels = np.array([1, 0, 1], np.uint32)
    res, _ = _one(ix, q, 10, labels)
    assert _ids(res) == [2, 0]
    assert all(int(x) == PAD for x in res[0][2:]) and all(v == np.float32(3.402823e38) for v in res[1][2:])
    res, _ = _one(ix, q, 10, np.ones(3, np.uint32), excluded=np.array([1], np.uint32))     # ... and the same through the exclusion set
    assert _ids(res) == [2, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the GPU inputs reach the edges they are there for
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_gpu_inputs_reach_their_edges(request, fixture):
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = np.ascontiguousarray(q[:NQ])
    L = 37
    tr = _traces(fixture, ix, q, L)
    rank0 = np.array([t.wl_ids[0] for t in tr], np.uint64)
    short = absent = late = 0
    for tname, bname in LI.CASES:
        labels = LI.table(tname, ix, rank0)
        any_, all_ = LI.batch(bname, NQ)
        ids, d, matched, st, first = LR.collect_all(tr, labels, any_, all_, K, L, int(ix.medoid))
        short += int((ids == LR.PAD_ID).any(axis=1).sum())
        late += int((first > 1).sum())
        for i, t in enumerate(tr):
            absent += len(set(int(x) for x in ids[i] if int(x) != PAD) - set(int(x) for x in t.wl_ids))
        if tname == "nobody":
            assert (ids == LR.PAD_ID).all() and (matched == 0).all() and (first == 0).all()
        if tname == "one_node":
            assert np.array_equal(ids[:, 0], rank0) and (ids[:, 1:] == LR.PAD_ID).all() and (matched >= 1).all()
        if bname == "mixed":
            ids_x, d_x, _ = XR.Reference(ix).search(q[::3], K, L, "exact")
            assert np.array_equal(ids[::3], ids_x) and np.array_equal(_bits(d[:, ::3]), _bits(d_x))
    assert short > 0 and absent > 0 and late > 0, (short, absent, late)
