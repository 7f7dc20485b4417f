"""Range search on the exact-distance walk (CANON 19), without a GPU: the CPU reference of tests/range_reference.py against
exact_reference (the recorded walk is today's walk, bit for bit), hand-derived answers on the toy inputs, and the edges the GPU inputs of
tests/test_gpu_range.py must reach."""
import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
import exact_reference as XR
import labels_reference as LR
import range_inputs as RI
import range_reference as RR

NQ = 32
K = 10
LS = (10, 37, 152)
_CACHE = {}


def _ref(name, ix):
    if ("ref", name) not in _CACHE:
        _CACHE[("ref", name)] = RR.Reference(ix)
    return _CACHE[("ref", name)]


def _traces(name, ix, q, L):
    key = (name, q.shape, L)
    if key not in _CACHE:
        _CACHE[key] = _ref(name, ix).evaluated_all(q, L)
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _get(request, fixture):
    ix, q, _, _ = request.getfixturevalue(fixture)
    return ix, np.ascontiguousarray(q[:NQ])


@pytest.mark.parametrize("fixture", ("small_u8", "small_f32", "small_i8"))
@pytest.mark.parametrize("L", LS)
def test_the_recorded_walk_is_the_exact_reference_bit_for_bit(request, fixture, L):
    """Top-k, the four counters and the candidate log of the recorded walk are those of exact_reference / labels_reference; every evaluation is in
    the record once."""
    ix, q = _get(request, fixture)
    tr = _traces(fixture, ix, q, L)
    ids_x, d_x, st_x = XR.Reference(ix).search(q, K, L, "exact")
    lab = LR.Reference(ix)
    for i, t in enumerate(tr):
        n = min(K, len(t.wl_ids))
        assert np.array_equal(ids_x[i, :n], t.wl_ids[:n].astype(np.uint64)) and (ids_x[i, n:] == RR.PAD_ID).all()
        assert np.array_equal(_bits(d_x[:n, i]), _bits(t.wl_dists[:n]))
        assert tuple(st_x[i]) == tuple(t.stats)
        assert sum(len(S) for _, S, _ in t.iters) == t.stats[2]                   # dist_evals: every evaluated survivor is recorded
        assert [it for it, _, _ in t.iters] == sorted({it for it, _, _ in t.iters})
        if i < 4:
            w = lab.walk(q[i], L)
            assert np.array_equal(w.log, t.log) and w.stats == t.stats
            assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2])) for a, b in zip(w.merged, t.iters))


@pytest.mark.parametrize("fixture", ("small_u8", "small_f32", "small_i8"))
def test_the_radii_reach_their_edges(request, fixture):
    ix, q = _get(request, fixture)
    ref = _ref(fixture, ix)
    r = {n: RI.radii(n, ref, ix, q) for n in RI.NAMES}
    assert (r["none"] == -1).all() and np.isinf(r["all"]).all()
    assert (r["mixed"][::3] == -1).all() and np.isnan(r["mixed"][1]) and np.isfinite(r["mixed"][2]) and r["mixed"][2] == r["rank100"][2]
    assert (r["rank5"] <= r["rank100"]).all() and (r["rank100"] <= r["rank400"]).all() and (r["rank5"] >= 0).all()
    over64 = False
    for L in LS:
        tr = _traces(fixture, ix, q, L)
        # no range at all; the NaN query and the negative ones of the mixed batch
        *_, counts, offered = RR.collect_all(tr, r["none"], 512)
        assert not counts.any() and not offered.any()
        *_, counts, offered = RR.collect_all(tr, r["mixed"], 512)
        assert not counts[::3].any() and counts[1] == 0 and counts[2] > 0
        # the rank-N point is AT the radius: a walk that meets it logs it (the compare is <=)
        for i, t in enumerate(tr):
            ids, d, _ = RR.hits(t, r["rank5"][i])
            every = np.concatenate([dd for _, _, dd in t.iters])
            assert (_bits(every) == _bits(r["rank5"][i:i + 1])[0]).any() == (_bits(d) == _bits(r["rank5"][i:i + 1])[0]).any()
        # rank100: more than 64 hits for some query, over more than one iteration
        for i, t in enumerate(tr):
            ids, d, its = RR.hits(t, r["rank100"][i])
            over64 |= len(ids) > 64 and len(set(its.tolist())) > 1
        # rank400 overflows cap = 64 for every query; cap = 512 holds every query
        *_, c64, o400 = RR.collect_all(tr, r["rank400"], 64)
        *_, c512, o512 = RR.collect_all(tr, r["rank400"], 512)
        assert (o400 > 64).all() and (o512 <= 512).all() and (c64 <= 64).all() and np.array_equal(o400, o512), (L, o400.min(), o400.max())
    assert over64
    # all: every evaluation, still under the largest capacity
    *_, counts, offered = RR.collect_all(_traces(fixture, ix, q, 152), r["all"], 4096)
    assert offered.max() < 4096 and np.array_equal(offered, [t.stats[2] for t in _traces(fixture, ix, q, 152)])


def _one(ix, q, L, radius, cap=512, excluded=None):
    t = RR.Reference(ix).evaluated(q[0], L)
    return RR.collect(t, radius, cap, excluded), t


@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed65_puts_a_hit_in_seed_slot_64(variant, dtype, D):
    """The 65-id seed list: with every node in range, iteration 1 offers 65 hits and the last of them is node 64, the one no lane holds."""
    ix, q = E.seed65(dtype, variant, D)
    (ids, d, offered, count), t = _one(ix, q, 10, np.inf)
    it, S, dd = t.iters[0]
    assert it == 1 and len(S) == 65 and int(S[64]) == E.SEED65_LAST
    assert int(E.SEED65_LAST) in ids.tolist() and offered >= 65
    # ... and with a radius that only node 64's distance meets (variant best: it is strictly the nearest of the seed list)
    if variant == "best":
        (ids1, _, off1, _), _ = _one(ix, q, 10, dd[64])
        h_ids, _, h_it = RR.hits(t, dd[64])
        assert int(h_ids[0]) == E.SEED65_LAST and h_it[0] == 1


def test_chain_puts_a_hit_in_the_cap_iteration():
    """The chain ends at the iteration cap: its last survivor is evaluated, never merged into the worklist, and is a hit all the same."""
    ix, q = E.chain()
    L = 10
    (ids, d, offered, count), t = _one(ix, q, L, np.inf)
    it, S, dd = t.iters[-1]
    assert it == L + XR.EXTRA_ITERS - 1 == t.stats[0] and len(S) == 1
    assert int(S[0]) not in t.wl_ids.tolist() and int(S[0]) in ids.tolist()
    assert offered == t.stats[2] == count
    # the radius of that node alone: one hit, the nearest the walk ever saw
    (ids1, d1, off1, c1), _ = _one(ix, q, L, dd[0])
    assert ids1.tolist() == [int(S[0])] and off1 == 1 and _bits(d1)[0] == _bits(dd)[0]


def test_short_worklist_evaluates_three_nodes_once():
    """Node 1's row lists node 2 twice, but every id is in the filter after iteration 1: three evaluations, three hits, none of them twice
    (offered == count; the row that IS evaluated twice is beam_inputs.row_dup, below)."""
    ix, q = E.short_worklist()
    (ids, d, offered, count), t = _one(ix, q, 10, np.inf)
    assert offered == t.stats[2] == count == 3 and sorted(ids.tolist()) == [0, 1, 2]
    # an excluded node is no hit
    (ids_x, _, off_x, _), _ = _one(ix, q, 10, np.inf, excluded=np.array([2], np.uint32))
    assert sorted(ids_x.tolist()) == [0, 1] and off_x == 2


def test_row_dup_offers_a_duplicate_that_the_sort_drops():
    """Node 2 stands twice in ONE row: both copies pass the filter, both are evaluated and offered, the answer holds node 2 once."""
    ix, q = BI.row_dup()
    (ids, d, offered, count), t = _one(ix, q, 10, np.inf)
    assert offered == t.stats[2] and offered == count + 1 and sorted(ids.tolist()) == sorted(set(ids.tolist()))
    h_ids, _, _ = RR.hits(t, np.inf)
    assert h_ids.tolist().count(2) == 2 and ids.tolist().count(2) == 1
    (ids_x, _, off_x, _), _ = _one(ix, q, 10, np.inf, excluded=np.array([2], np.uint32))
    assert 2 not in ids_x.tolist() and off_x == offered - 2


def test_tie_heavy_orders_equal_distances_by_id(small_u8):
    ix, q, _, _ = small_u8
    ixt, qt = E.tie_heavy(ix, q, 8)
    ref = RR.Reference(ixt)
    seen = False
    for i in range(qt.shape[0]):
        ids, d, offered, count = RR.collect(ref.evaluated(qt[i], 37), np.inf, 4096)
        b = _bits(d)
        assert (np.diff(b.astype(np.int64)) >= 0).all()
        same = b[1:] == b[:-1]
        assert (ids[1:][same] > ids[:-1][same]).all()
        seen |= bool(same.any())
    assert seen


def test_the_first_cap_hits_in_evaluation_order_are_kept(small_u8):
    ix, q, _, _ = small_u8
    t = _traces("small_u8", ix, np.ascontiguousarray(q[:NQ]), 37)[0]
    h_ids, h_d, _ = RR.hits(t, np.inf)
    ids, d, offered, count = RR.collect(t, np.inf, 64)
    assert offered == len(h_ids) > 64 and count <= 64
    assert set(ids.tolist()) == set(h_ids[:64].tolist())
