"""The inputs of tests/edge_inputs.py reach the edges they are named for -- asserted on the CPU references alone (tests/exact_reference.py,
tests/inmemory_reference.py), so that an input that stops reaching its edge after a generator change fails HERE instead of turning a GPU
test into a silent pass.  These are conditions, not measurements.  The reference compositions are pinned to Oracle.search on the new inputs
the way tests/test_exact_mode.py pins them on the fixtures."""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as E
import exact_reference as X
import inmemory_reference as M
from oracle import oracle as O

BIG_DIST = X.BIG_DIST
TIE_FIXTURES = ("small_u8", "small_i8", "small_f32")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def _pinned_to_the_oracle(ix, q, k, L):
    """Both compositions of the BANG_Base walk equal Oracle.search bit for bit: ids, distance bits, per-query statistics."""
    want = O.Oracle(ix).search(q, k, L, with_stats=True)
    assert _same(X.Reference(ix).search(q, k, L, "pq"), want)
    assert _same(M.Reference(ix).search(q, k, L, "base"), want)


# ---------------------------------------------------------------------------------------------------------------------
# (a) toys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
@pytest.mark.parametrize("name", sorted(E.TOYS))
def test_toy_compositions_equal_the_oracle(name, dtype, D):
    ix, q = E.toy_named(name, dtype, D)
    assert (ix.dtype, ix.D, ix.m) == (dtype, D, D // 4) and q.dtype == E.NP_DTYPE[dtype]
    for L in (3, 10):
        _pinned_to_the_oracle(ix, q, L, L)


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
@pytest.mark.parametrize("name", sorted(E.TOYS))
def test_toy_walks_expand_a_row_of_pads_only(name, dtype, D):
    """The leaves of the toy graphs have degree 0.  At L = 10 the BANG_Base walk expands one: no node is expanded twice, and the walk logs more
    candidates than there are nodes with a neighbour."""
    ix, q = E.toy_named(name, dtype, D)
    _, _, st = O.Oracle(ix).search(q, 3, 10, with_stats=True)
    assert int(st[0][1]) > int((ix.degrees() > 0).sum())


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_toy_distances_are_the_level_differences(dtype, D):
    """Exact and PQ distance of node i are both D levels[i]^2, in every layout: equal levels tie in both."""
    adj, levels = E.TOYS["head_tie"]
    ix, q = E.toy(adj, levels, dtype, D)
    r = X.Reference(ix)
    ids = np.arange(ix.N, dtype=np.uint32)
    want = (D * np.asarray(levels, np.int64) ** 2).astype(np.float32)
    assert np.array_equal(r.exact(ids, q[0]), want)
    assert np.array_equal(r.orc.pqdist(r.orc.lut_build(q[0]), ids), want)


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_toy_ties_decide_the_walk(dtype, D):
    # every tie toy has two equal distances among its results
    for name in ("tie", "medoid_tie", "head_tie"):
        ix, q = E.toy_named(name, dtype, D)
        for mode in X.MODES:
            assert E.ties_in_top(X.Reference(ix).search(q, 10, 10, mode)[1], 10).all(), (name, mode)
    # "tie": the worklist keeps the tied pair in merge order, the re-rank in candidate order
    ix, q = E.toy_named("tie", dtype, D)
    ex, pq = (X.Reference(ix).search(q, 10, 10, mode) for mode in ("exact", "pq"))
    assert ex[0][0].tolist()[:6] == [4, 5, 1, 3, 2, 0] and pq[0][0].tolist()[:6] == [4, 5, 1, 2, 3, 0]
    # "tie" / "head_tie" at L = 3: the two parent rules expand different nodes
    for name in ("tie", "head_tie"):
        ix, q = E.toy_named(name, dtype, D)
        base, inm = (M.Reference(ix).search(q, 3, 3, mode) for mode in M.MODES)
        assert not np.array_equal(base[2], inm[2]), name
    # "head_tie": node 4 ties the worklist's first unvisited entry (node 2) and the entry is expanded first -- 5 is found before 7
    ix, q = E.toy_named("head_tie", dtype, D)
    assert X.Reference(ix).search(q, 3, 3, "exact")[0][0].tolist() == [8, 5, 1]


# ---------------------------------------------------------------------------------------------------------------------
# (b) the cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_chain_runs_to_the_cap(dtype, D):
    ix, q = E.chain(dtype, D)
    for L in (10, 37):
        cap = L + 49
        ids, d, st = X.Reference(ix).search(q, 10, L, "exact")
        assert st[0].tolist() == [cap, cap + 1, cap + 1, cap + 1]
        # node `cap` is the survivor of the last iteration: evaluated, never merged (CANON 6)
        assert ids[0].tolist() == [cap - 1 - r for r in range(10)]
        assert d[:, 0].tolist() == [float(D * (255 - (cap - 1 - r)) ** 2) for r in range(10)]
        assert M.Reference(ix).search(q, 10, L, "inmemory")[2][0].tolist() == [L + 119, L + 120, L + 120, L + 120]
        _pinned_to_the_oracle(ix, q, 10, L)


# ---------------------------------------------------------------------------------------------------------------------
# (c) padding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_short_worklist_is_padded(dtype, D):
    ix, q = E.short_worklist(dtype, D)
    ids, d, st = X.Reference(ix).search(q, 10, 16, "exact")
    assert ids[0].tolist() == [1, 2, 0] + [int(E.ID_PAD)] * 7
    assert d[:3, 0].tolist() == [D * 100.0, D * 400.0, D * 900.0]
    assert np.array_equal(d[3:, 0].view(np.uint32), np.full(7, BIG_DIST, np.float32).view(np.uint32))
    assert st[0].tolist() == [3, 3, 3, 7]                                # the self-loop and the duplicate are fetched, never evaluated
    _pinned_to_the_oracle(ix, q, 10, 16)


# ---------------------------------------------------------------------------------------------------------------------
# (d) 65 seeds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
def test_seed65_evaluates_65_seeds_and_the_last_one_decides(dtype, D):
    res = {}
    for variant in E.SEED65_VARIANTS:
        ix, q = E.seed65(dtype, variant, D)
        r = X.Reference(ix)
        assert ix.R == 64 and int(ix.degrees()[ix.medoid]) == 64
        seeds = np.concatenate([[ix.medoid], r.adjacency(ix.medoid)]).astype(np.uint32)
        assert len(seeds) == 65 and int(seeds[64]) == E.SEED65_LAST
        # dist_evals of iteration 1: every seed passes the empty filter
        assert len(O.filter_ids(np.zeros(O.BF_MEMORY, np.uint8), seeds)) == 65
        d = r.exact(seeds, q[0])
        first64 = np.where(seeds[:64] == ix.medoid, np.inf, d[:64])
        assert int(seeds[int(np.argmin(first64))]) == E.SEED65_BEST_OF_64 and (first64 == first64.min()).sum() == 2
        if variant == "best":
            assert d[64] < first64.min()
        elif variant == "tie":
            assert d[64] == first64.min()
        else:
            assert d[64] > first64.min()
        for L in (4, 10, 37):
            _pinned_to_the_oracle(ix, q, L, L)
        res[variant] = {mode: X.Reference(ix).search(q, 4, 4, mode) for mode in X.MODES}
        res[variant]["inmemory"] = M.Reference(ix).search(q, 4, 4, "inmemory")
    for mode in ("exact", "pq", "inmemory"):
        # the 65th seed is expanded first only when it is strictly best: at L = 4 that decides what the search finds
        assert res["best"][mode][0][0].tolist() == [74, 69, 64, 70], mode
        assert res["tie"][mode][0][0].tolist() == [75, 72, 65, 66], mode
        assert res["worse"][mode][0][0].tolist() == [75, 72, 65, 66], mode


@pytest.mark.parametrize("dtype,D", E.DEGREE64_LAYOUTS)
def test_degree64_expands_a_full_row(dtype, D):
    ix, q = E.degree64(dtype, D)
    assert ix.R == 64 and int(ix.degrees()[E.DEGREE64_NODE]) == 64 and int(ix.degrees()[ix.medoid]) == 1
    for L in (5, 37):
        ids, _, st = O.Oracle(ix).search(q, 5, L, with_stats=True)
        assert int(st[0][3]) >= 64 + 2                                       # fetched: the seed list and the full row
        assert ids[0].tolist()[:2] == [67, 66]
        _pinned_to_the_oracle(ix, q, 5, L)


# ---------------------------------------------------------------------------------------------------------------------
# (e) ties everywhere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_heavy_inputs_tie(name, request):
    ix0, q0, _, _ = request.getfixturevalue(name)
    ix, q = E.tie_heavy(ix0, q0)
    assert q.shape[0] == 16 and np.array_equal(ix.adjacency(), ix0.adjacency()) and np.array_equal(ix.degrees(), ix0.degrees())
    v = ix.vectors()
    if ix.dtype == "float":                                              # small integers: every distance is exact in float
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 4 and np.array_equal(q, np.rint(q))
    else:
        assert (v.min(), v.max()) == {"uint8": (0, 3), "int8": (-2, 1)}[ix.dtype]
    k, L = 10, 37
    ex, pq = (X.Reference(ix).search(q, k, L, mode) for mode in X.MODES)
    inm = M.Reference(ix).search(q, k, L, "inmemory")
    for ref in (ex, pq, inm):
        assert 2 * int(E.ties_in_top(ref[1], k).sum()) >= q.shape[0]     # ties among the first k of at least half of the queries
    assert (ex[0] != pq[0]).any(axis=1).sum() > 0                        # the worklist's order is not the re-rank's
    assert (pq[2] != inm[2]).any(axis=1).sum() > 0                       # the two parent rules walk differently
    assert not (ex[0] == E.ID_PAD).any()
    _pinned_to_the_oracle(ix, q, k, L)


def test_a_smaller_k_is_a_prefix(small_u8):
    """edge_inputs.first_k: in every mode, k only cuts the final list."""
    ix, q = E.tie_heavy(*small_u8[:2], n_queries=4)
    L = 37
    for ref, mode in ((X.Reference(ix), "exact"), (X.Reference(ix), "pq"), (M.Reference(ix), "inmemory"), (M.Reference(ix), "base")):
        full = ref.search(q, L, L, mode)
        for k in (1, 10):
            assert _same(ref.search(q, k, L, mode), E.first_k(full, k)), (mode, k)
    ix, q = E.short_worklist()
    full = X.Reference(ix).search(q, 16, 16, "exact")
    assert _same(X.Reference(ix).search(q, 10, 16, "exact"), E.first_k(full, 10))


# ---------------------------------------------------------------------------------------------------------------------
# (f) the ends of the 8-bit ranges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_extreme_values_reach_the_top_of_the_integer_range(dtype):
    ix, q = E.extreme(dtype)
    assert ix.D == 256 and q.shape[0] <= 16
    v = ix.vectors()
    assert sorted(np.unique(v).tolist()) == ([0, 255] if dtype == "uint8" else [-128, 127]) == sorted(np.unique(q).tolist())
    for L, floor in ((37, 16_000_000), (152, 16_646_400)):
        ids, d, _ = X.Reference(ix).search(q, L, L, "exact")
        top = float(d[d < BIG_DIST].max())
        assert floor <= top < (1 << 24), (L, top)                       # L = 152 holds nearly every node: all-low against all-high is there
        assert not (ids == E.ID_PAD).any()
    _pinned_to_the_oracle(ix, q, 10, 37)


# ---------------------------------------------------------------------------------------------------------------------
# (g) shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_shape_list_covers_the_layouts():
    eight = {s[1] for s in E.SHAPES if s[2] != "float"}
    flt = {s[1] for s in E.SHAPES if s[2] == "float"}
    assert {16, 32, 256} <= eight and {4, 20, 68, 132, 252, 256} <= flt
    assert {8, 32, 64} <= {s[3] for s in E.SHAPES}
    assert {"uint8", "int8", "float"} == {s[2] for s in E.SHAPES}
    assert all(s[5] <= 16 for s in E.SHAPES if s[1] == 256)
    assert {s[1] // 16 for s in E.SHAPES if s[2] != "float"} == {1, 2, 16}          # G: lanes per 8-bit survivor


@pytest.mark.parametrize("shape", E.SHAPES, ids=E.shape_id)
def test_shapes_build_and_run_through_the_references(shape, libbang):
    ix, q = E.shape_index(shape)
    N, D, dtype, R, m, Q = shape
    assert (ix.N, ix.D, ix.dtype, ix.R, ix.m, q.shape) == (N, D, dtype, R, m, (Q, D))
    libbang.bang_search_can_rerank.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32]
    assert libbang.bang_search_can_rerank(O.DTYPE_CODE[dtype], D, ix.entry_len, 0) == 1       # a layout the exact kernel evaluates
    ids, d, st = X.Reference(ix).search(q, 10, 37, "exact")
    assert not (ids == E.ID_PAD).any() and np.all(np.diff(d, axis=0) >= 0)
    assert (st[:, 0] < 37 + 49).all()
    _pinned_to_the_oracle(ix, q, 10, 37)


# ---------------------------------------------------------------------------------------------------------------------
# every input with a search-kernel instance fits the host-paced form
# ---------------------------------------------------------------------------------------------------------------------
def test_lds_holds_the_host_paced_form_on_every_input(request, libbang):
    """tests/test_gpu_base_edges.py skips a host-paced case that reports search_kernel == 0 as "no CPU-writable device memory".  The engine's other
    reason to decline the form, LDS, is ruled out here, in host code, for every input and up to the longest worklist that file runs on them;
    the layouts it treats as LUT-path ones are those without an instance."""
    import base_forms as F
    inputs = [E.toy_named("head_tie", dtype, D)[0] for dtype, D in E.TOY_LAYOUTS]              # (every toy, chain, seed65, degree64: D / 4 chunks)
    inputs += [E.shape_index(s)[0] for s in E.SHAPES]
    inputs += [E.tie_heavy(*request.getfixturevalue(name)[:2])[0] for name in TIE_FIXTURES]
    inputs += [E.extreme("uint8")[0]]
    for ix in inputs:
        for L in (3, 10, 16, F.EDGE_MAX_L):
            assert (F.host_paced_waves(ix, L) >= 1) == (ix.D < 132), (ix.dtype, ix.D, ix.m, L)
