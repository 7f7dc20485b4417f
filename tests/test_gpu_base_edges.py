"""The edge inputs of tests/edge_inputs.py through every form of the BANG_Base PQ walk (tests/base_forms.py: the self-paced search kernel with
the graph in HBM, the pulled-rows form in its three row placements, the host-paced walker forms, the launch-per-iteration loop; on LUT-path
layouts the loop and search_lut_kernel) -- against oracle.Oracle.search, to which tests/test_edge_inputs.py pins these inputs: ids, distance bits
and the per-query counters, bit for bit.  A row of pads only, a full 64-id row, a tie between the best survivor and the worklist's head with the
next row already requested, a walk to the iteration cap, a worklist shorter than k and distances just under 2^24 reach forms that met none of
them before.  Which kernel serves a pairing is asserted (bang_get_stats), never branched on."""
import numpy as np
import pytest

import base_forms as F
import edge_inputs as E
from exact_reference import BIG_DIST

pytestmark = pytest.mark.gpu

TIE_FIXTURES = ("small_u8", "small_i8", "small_f32")
GROUPS = tuple(F.GROUPS)
_REF = {}


def _oracle(key, ix, q, k, L):
    """Oracle.search(..., with_stats=True), once per (input, k, L)."""
    from oracle import oracle as O
    if (key, k, L) not in _REF:
        _REF[(key, k, L)] = O.Oracle(ix).search(q, k, L, with_stats=True)
    return _REF[(key, k, L)]


def _instance(ix) -> int:
    """psz * 100 + mp / 4 of the layout's search-kernel instance; 0 on the LUT path."""
    from bang_amd import binding as B
    psz, mp = B.pq_layout(ix.chunk_off, ix.D, ix.m)
    return psz * 100 + mp // 4 if psz else 0


def _walk(key, ix, q, group, runs, monkeypatch, check=None):
    """Every form of `group` (a group of base_forms.GROUPS, or one of LUT_FORMS on a LUT-path layout) at every (k, L) of `runs`: parity with the
    oracle, the statistics of the form, and check(e, form, got, stats, k, L) for what the input is there for."""
    lut = group in F.LUT_FORMS
    assert (_instance(ix) == 0) == lut, (key, group)
    assert lut or max(L for _, L in runs) <= F.EDGE_MAX_L                # (up to there tests/test_edge_inputs.py pins that LDS holds every form)
    for form in ((group,) if lut else F.forms_of(group, ix.dtype, ix.D, ix.R, ix.N)):
        with F.open_engine(ix, form, monkeypatch) as e:
            for k, L in runs:
                got = F.run(e, form, q, k, L)
                F.assert_same(got, _oracle(key, ix, q, k, L), form)
                s = F.assert_form(e, form, ix, q.shape[0], L)
                if check is not None:
                    check(e, form, got, s, k, L)
                e.free()
            e.unload()


def _groups_for(D):
    """Parameter lists are made without the library: in these inputs the layouts of 132 and more dimensions are the LUT-path ones (chunks of 4
    dimensions: more than 32 of them have no LDS instance); _walk asserts it."""
    return F.LUT_FORMS if D >= 132 else GROUPS


def _params(layouts, *more):
    """(dtype, D, *more, group) for every layout and every group the layout has."""
    out = []
    for dtype, D in layouts:
        for rest in (more[0] if more else [()]):
            rest = rest if isinstance(rest, tuple) else (rest,)
            for g in _groups_for(D):
                out.append(pytest.param(dtype, D, *rest, g, id="-".join([dtype, f"D{D}", *map(str, rest), g])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (a) toys: ties, and rows of pads only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,name,group", _params(E.TOY_LAYOUTS, sorted(E.TOYS)))
def test_toy_graphs_and_rows_of_pads_only(dtype, D, name, group, monkeypatch):
    """Distance ties; the leaves have degree 0 and at L = 10 every walk expands one (tests/test_edge_inputs.py).  head_tie: the self-paced forms
    have requested the next row before the merge decides the parent (`bd < head.d`, strict) -- in the pulled forms from host memory and from HBM."""
    ix, q = E.toy_named(name, dtype, D)
    assert _instance(ix) in ((0,) if D == 256 else (404, 408))
    _walk(("toy", name, dtype, D), ix, q, group, ((3, 3), (3, 10), (10, 10)), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the iteration cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,group", _params(E.TOY_LAYOUTS))
def test_chain_runs_to_the_cap(dtype, D, group, monkeypatch):
    ix, q = E.chain(dtype, D)

    def check(e, form, got, s, k, L):
        cap = L + 49
        assert got[2][0].tolist()[1:] == [cap + 1, cap + 1, cap + 1]
        if F.reports_iterations(form):
            assert int(got[2][0][0]) == cap
        c_ids, c_cnt = e.candidate_log(1, L)
        assert int(c_cnt[0]) == L + 50 and c_ids[0].tolist() == list(range(L + 50))
        if form == "pull_host":
            assert s["pulled_bytes"] == 256 * (L + 49)

    _walk(("chain", dtype, D), ix, q, group, ((10, 10), (10, 37)), monkeypatch, check)


# ---------------------------------------------------------------------------------------------------------------------
# (c) a worklist shorter than k
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,group", _params(E.TOY_LAYOUTS))
def test_short_worklist_is_padded(dtype, D, group, monkeypatch):
    """Three candidates for k = 10: the fused re-rank and the re-rank launch (the two forms of group self) both pad seven results."""
    ix, q = E.short_worklist(dtype, D)

    def check(e, form, got, s, k, L):
        assert got[0][0].tolist() == [1, 2, 0] + [int(E.ID_PAD)] * 7
        assert np.array_equal(got[1][3:, 0].view(np.uint32), np.full(7, BIG_DIST, np.float32).view(np.uint32))

    _walk(("short", dtype, D), ix, q, group, ((10, 16),), monkeypatch, check)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the 65-id seed list, and an expanded row of 64 ids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,variant,group", _params(E.SEED65_LAYOUTS, E.SEED65_VARIANTS))
def test_seed_list_of_65(dtype, D, variant, group, monkeypatch):
    ix, q = E.seed65(dtype, variant, D)
    want = [74, 69, 64, 70] if variant == "best" else [75, 72, 65, 66]

    def check(e, form, got, s, k, L):
        if (k, L) == (4, 4):
            assert got[0][0].tolist() == want

    _walk(("seed65", variant, dtype, D), ix, q, group, ((4, 4), (10, 10), (10, 37)), monkeypatch, check)


@pytest.mark.parametrize("dtype,D,group", _params(E.DEGREE64_LAYOUTS))
def test_expanded_node_of_degree_64(dtype, D, group, monkeypatch):
    ix, q = E.degree64(dtype, D)
    assert int(ix.degrees()[E.DEGREE64_NODE]) == 64

    def check(e, form, got, s, k, L):
        assert int(got[2][0][3]) >= 64 + 2                      # fetched: the seed list and the full row

    _walk(("deg64", dtype, D), ix, q, group, ((5, 5), (5, 37)), monkeypatch, check)


# ---------------------------------------------------------------------------------------------------------------------
# (e) ties everywhere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_heavy_vectors_and_pivots(name, group, request, monkeypatch):
    ix, q = E.tie_heavy(*request.getfixturevalue(name)[:2])
    assert E.ties_in_top(_oracle(("tie_heavy", name), ix, q, 10, 37)[1], 10).any()
    _walk(("tie_heavy", name), ix, q, group, ((10, 37), (37, 37)), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# (f) distances just under 2^24 (a LUT-path layout)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", F.LUT_FORMS)
@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_extreme_values_reach_the_top_of_the_integer_range(dtype, form, monkeypatch):
    ix, q = E.extreme(dtype)

    def check(e, form, got, s, k, L):
        if L == 152:
            d = got[1]
            assert 16_646_400 <= float(d[d < BIG_DIST].max()) < (1 << 24)

    _walk(("extreme", dtype), ix, q, form, ((10, 37), (152, 152)), monkeypatch, check)


# ---------------------------------------------------------------------------------------------------------------------
# (g) the vector layouts at either end of what the kernels evaluate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,group", [pytest.param(s, g, id=f"{E.shape_id(s)}-{g}") for s in E.SHAPES for g in _groups_for(s[1])])
def test_layouts_of_the_shape_list(shape, group, monkeypatch):
    ix, q = E.shape_index(shape)
    _walk(("shape", shape), ix, q, group, ((10, 37),), monkeypatch)
