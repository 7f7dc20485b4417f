"""The BANG_Inmemory search semantics (option "semantics" = 1, search_inmem_kernel of csrc/bang_search.hip) beyond the four fixtures: the 65-id
seed list, tie-heavy distances, the PQ layouts of tests/edge_inputs.SHAPES and of tests/test_gpu_random_configs.CASES, k = 1, k = L and k > 64
-- against the CPU reference composed from the oracle's stages (tests/inmemory_reference.py), bit for bit: ids, distance bits and the four
per-query counters.  A layout bang_alloc refuses for semantics = 1 is asserted to be refused, with its message.  The BANG_Base device-graph
kernel runs the seed-list and tie inputs too, against Oracle.search."""
import numpy as np
import pytest

import edge_inputs as E
from inmemory_reference import Reference
from test_gpu_random_configs import CASES

pytestmark = pytest.mark.gpu

TIE_FIXTURES = ("small_u8", "small_i8", "small_f32")
# semantics = 1 has no LUT-path kernel: it needs the pivot table in LDS, with every chunk padded to 1, 2, 4 or 8 dimensions x 256 floats.
# 18-dimension chunks have no such layout, and from D = 132 up the table of these shapes is larger than LDS.
NO_LDS_TABLE = r"semantics = 1 \(inmemory\) needs the LDS-resident pivot table"
_REF = {}


def _reference(key, ix, q, L):
    """The reference at k = L; a smaller k is a prefix of it (edge_inputs.first_k)."""
    if (key, L) not in _REF:
        _REF[(key, L)] = Reference(ix).search(q, L, L, "inmemory")
    return _REF[(key, L)]


def _engine(ix, **opts):
    import bang_amd
    opts.setdefault("semantics", bang_amd.SEMANTICS_INMEMORY)
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, **opts)
    e.load_index(ix)
    return e


def _run(e, q, k, L, Q=None):
    Q = q.shape[0] if Q is None else Q
    e.set_searchparams(k, L)
    e.alloc(Q)
    e.init(q.shape[0])
    ids, d = e.query(q)
    return ids, d, e.query_counters(q.shape[0])


def _assert_same(got, want):
    ids, d, st = got
    ids_r, d_r, st_r = want
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
    assert np.array_equal(st, st_r)                       # iterations, candidates, dist_evals, fetched


def _ks(L):
    return sorted({1, min(10, L), L})


def _check(e, key, ix, q, L, ks=None):
    ref = _reference(key, ix, q, L)
    for k in (_ks(L) if ks is None else ks):
        _assert_same(_run(e, q, k, L), E.first_k(ref, k))
        assert e.stats()["search_kernel"] == 1
        e.free()


def _assert_refused(ix, q, k, L, message):
    import bang_amd
    with _engine(ix) as e:
        e.set_searchparams(k, L)
        with pytest.raises(bang_amd.BangError, match=message):
            e.alloc(q.shape[0])


@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed_list_of_65(variant, dtype, D):
    ix, q = E.seed65(dtype, variant, D)
    with _engine(ix) as e:
        for L in (4, 10, 37):
            _check(e, ("seed65", variant, dtype, D), ix, q, L)
        _run(e, q, 4, 4)
        c_ids, _ = e.candidate_log(1, 4, 120)
        assert int(c_ids[0][1]) == (E.SEED65_LAST if variant == "best" else E.SEED65_BEST_OF_64)     # the first parent
        e.free()


@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_heavy_vectors_and_pivots(name, request):
    ix, q = E.tie_heavy(*request.getfixturevalue(name)[:2])
    with _engine(ix) as e:
        _check(e, ("tie_heavy", name), ix, q, 37)
        _check(e, ("tie_heavy", name), ix, q, 152, ks=(100, 152))      # k > 64


@pytest.mark.parametrize("shape", E.SHAPES, ids=E.shape_id)
def test_pq_layouts_of_the_shape_list(shape):
    ix, q = E.shape_index(shape)
    if shape[1] >= 132:
        _assert_refused(ix, q, 10, 37, NO_LDS_TABLE)
        return
    with _engine(ix) as e:
        _check(e, ("shape", shape), ix, q, 37)
        if shape[1] in (16, 68):
            _check(e, ("shape", shape), ix, q, 152, ks=(100,))


@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}-D{c[1]}-{c[2]}-R{c[3]}-m{c[4]}-Q{c[5]}-k{c[6]}-L{c[7]}" for c in CASES])
def test_random_config_shapes(case):
    """The index shapes of tests/test_gpu_random_configs.py (the same generator call), each at its own k and L, at k = 1 and at k = L."""
    from bang_amd import synth
    N, D, dtype, R, m, Q, k, L = case
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=min(10, k), n_clusters=8, seed=1000 + N + D, pq_iters=2)
    if D // m > 8:                                                         # 18 dimensions per chunk
        _assert_refused(ix, q, k, L, NO_LDS_TABLE)
        return
    with _engine(ix) as e:
        _check(e, ("random", case), ix, q, L, ks=sorted({1, k, L}))


def _base_walk_inputs():
    for dtype, D in E.SEED65_LAYOUTS:
        for variant in E.SEED65_VARIANTS:
            yield pytest.param("seed65", (dtype, D), variant, id=f"seed65-{dtype}-{variant}")
    for name in TIE_FIXTURES:
        yield pytest.param("tie_heavy", name, None, id=f"tie_heavy-{name}")


@pytest.mark.parametrize("kind,what,variant", list(_base_walk_inputs()))
def test_base_walk_on_the_seed_list_and_tie_inputs(kind, what, variant, request):
    """BANG_Base semantics, graph in HBM: the 65-id seed list and the ties reach search_kernel as well.  Against Oracle.search."""
    import bang_amd
    from oracle import oracle as O
    if kind == "seed65":
        ix, q = E.seed65(what[0], variant, what[1])
        cases = ((1, 4), (4, 4), (10, 10), (10, 37), (37, 37))
    else:
        ix, q = E.tie_heavy(*request.getfixturevalue(what)[:2])
        cases = ((1, 37), (10, 37), (37, 37), (100, 152))
    orc = O.Oracle(ix)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
        e.load_index(ix)
        for k, L in cases:
            _assert_same(_run(e, q, k, L), orc.search(q, k, L, with_stats=True))
            assert e.stats()["search_kernel"] == 1
            e.free()
