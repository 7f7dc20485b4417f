"""The exact-distance search kernel (option "distance" = 1, csrc/bang_search_exact.hip) at its edges: the inputs of tests/edge_inputs.py --
distance ties, the 65-id seed list, the iteration cap, a worklist shorter than k, the vector layouts at either end of what the kernel
evaluates, values at the ends of the 8-bit ranges -- with k = 1, k = L and k > 64, against the CPU reference composed from the oracle's
stages (tests/exact_reference.py).  Everything is compared bit for bit: ids, distance bits and the four per-query counters.
tests/test_edge_inputs.py asserts, without a GPU, that every input reaches the edge it is named for."""
import numpy as np
import pytest

import edge_inputs as E
from exact_reference import Reference

pytestmark = pytest.mark.gpu

TIE_FIXTURES = ("small_u8", "small_i8", "small_f32")
_REF = {}


def _reference(key, ix, q, L):
    """The reference at k = L; a smaller k is a prefix of it (edge_inputs.first_k)."""
    if (key, L) not in _REF:
        _REF[(key, L)] = Reference(ix).search(q, L, L, "exact")
    return _REF[(key, L)]


def _engine(ix, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT, **opts)
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
        s = e.stats()
        assert s["search_kernel"] == 1 and s["rerank_fused"] == 0
        e.free()


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
@pytest.mark.parametrize("name", sorted(E.TOYS))
def test_toy_graphs(name, dtype, D):
    ix, q = E.toy_named(name, dtype, D)
    with _engine(ix) as e:
        for L in (3, 10):
            _check(e, ("toy", name, dtype, D), ix, q, L)


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_chain_runs_to_the_cap(dtype, D):
    """The walk ends at iteration L + 49 with a survivor in hand: it is evaluated, logged as a candidate and NOT merged (CANON 6)."""
    ix, q = E.chain(dtype, D)
    with _engine(ix) as e:
        for L in (10, 37):
            cap = L + 49
            ref = _reference(("chain", dtype, D), ix, q, L)
            assert ref[2][0].tolist() == [cap, cap + 1, cap + 1, cap + 1] and int(ref[0][0][0]) == cap - 1
            for k in _ks(L):
                _assert_same(_run(e, q, k, L), E.first_k(ref, k))
                c_ids, c_cnt = e.candidate_log(1, L)
                assert int(c_cnt[0]) == cap + 1 and c_ids[0].tolist() == list(range(cap + 1))        # the chain, in order
                e.free()


@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_short_worklist_is_padded(dtype, D):
    ix, q = E.short_worklist(dtype, D)
    ref = _reference(("short", dtype, D), ix, q, 16)
    assert ref[0][0].tolist() == [1, 2, 0] + [int(E.ID_PAD)] * 13
    with _engine(ix) as e:
        _check(e, ("short", dtype, D), ix, q, 16)
        _check(e, ("short", dtype, D), ix, q, 152, ks=(100, 152))     # the second trip of the result loop is all padding


@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed_list_of_65(variant, dtype, D):
    ix, q = E.seed65(dtype, variant, D)
    with _engine(ix) as e:
        for L in (4, 10, 37):
            _check(e, ("seed65", variant, dtype, D), ix, q, L)
        _run(e, q, 4, 4)
        c_ids, c_cnt = e.candidate_log(1, 4)
        assert int(c_ids[0][1]) == (E.SEED65_LAST if variant == "best" else E.SEED65_BEST_OF_64)     # the first parent
        e.free()


@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_heavy_vectors(name, request):
    ix, q = E.tie_heavy(*request.getfixturevalue(name)[:2])
    with _engine(ix) as e:
        _check(e, ("tie_heavy", name), ix, q, 10)
        _check(e, ("tie_heavy", name), ix, q, 37)
        _check(e, ("tie_heavy", name), ix, q, 152, ks=(100, 152))      # k > 64: the result loop's second and third trips


def test_longest_worklist_with_k_equal_to_it(small_u8):
    ix, q = E.tie_heavy(*small_u8[:2], n_queries=4)
    with _engine(ix) as e:
        _check(e, ("tie_heavy", "small_u8", 4), ix, q, 512, ks=(512, 1))


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_extreme_values(dtype):
    ix, q = E.extreme(dtype)
    with _engine(ix) as e:
        _check(e, ("extreme", dtype), ix, q, 37)
        _check(e, ("extreme", dtype), ix, q, 152, ks=(100, 152))
    assert float(_reference(("extreme", dtype), ix, q, 152)[1].max()) == 16646400.0


@pytest.mark.parametrize("shape", E.SHAPES, ids=E.shape_id)
def test_vector_layouts(shape):
    ix, q = E.shape_index(shape)
    with _engine(ix) as e:
        _check(e, ("shape", shape), ix, q, 37)
        if shape[1] in (16, 256, 252, 20):
            _check(e, ("shape", shape), ix, q, 152, ks=(100,))


def _one_wave_inputs():
    for name in TIE_FIXTURES:
        yield pytest.param("tie_heavy", name, None, id=f"tie_heavy-{name}")
    for dtype, D in E.SEED65_LAYOUTS:
        for variant in E.SEED65_VARIANTS:
            yield pytest.param("seed65", (dtype, D), variant, id=f"seed65-{dtype}-{variant}")


@pytest.mark.parametrize("kind,what,variant", list(_one_wave_inputs()))
def test_one_wave_runs_every_query(kind, what, variant, request, monkeypatch):
    """BANG_SEARCH_MAX_WGS = BANG_SEARCH_MAX_WAVES = 1: a single wave runs the whole batch, query after query (the per-query state is reset)."""
    if kind == "tie_heavy":
        ix, q = E.tie_heavy(*request.getfixturevalue(what)[:2])
        key, Ls = ("tie_heavy", what), (37,)
    else:
        ix, q1 = E.seed65(what[0], variant, what[1])
        q = np.ascontiguousarray(np.repeat(q1, 5, axis=0))                 # the same query five times: the same answer five times
        key, Ls = ("seed65x5", variant) + what, (4, 37)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix) as e:
        for L in Ls:
            _check(e, key, ix, q, L)
