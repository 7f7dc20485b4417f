"""The exact scan's reference and inputs, on the CPU (tests/scan_reference.py, tests/scan_inputs.py): the two 8-bit reference paths agree, and
every crafted input reaches the edge it was made for -- before tests/test_gpu_scan.py holds the kernels to them."""
import numpy as np
import pytest

import scan_inputs as SI
import scan_reference as SR


def _fixture(request, name):
    ix, q = request.getfixturevalue(name)[:2]
    return ix, q


@pytest.mark.parametrize("name", ["small_u8", "small_i8"])
def test_the_two_8bit_reference_paths_agree_on_the_fixtures(request, name):
    ix, q = _fixture(request, name)
    a, b = SR.distances(ix, q), SR.distances_int(ix, q)
    assert a.shape == (q.shape[0], ix.N) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(SI.SMALL))
def test_the_two_8bit_reference_paths_agree_on_the_small_inputs(name):
    ix, q = SI.small(name)
    assert ix.N == SI.SMALL_N and ix.D == SI.SMALL[name][0] and q.shape == (SI.SMALL_Q, ix.D)
    a, b = SR.distances(ix, q), SR.distances_int(ix, q)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_extremes_reach_the_largest_sum(dtype):
    ix, q = SI.extremes(dtype)
    a, b = SR.distances(ix, q), SR.distances_int(ix, q)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(a.max()) == SI.EXTREME_MAX == 16646400 and float(a.min()) == 0.0
    assert SI.EXTREME_MAX < (1 << 24)
    # query 0 (all lowest): the even rows at 0, the odd rows at the largest sum, in id order inside each group
    ids, dists, matched = SR.answer(a, 64)
    assert list(ids[0]) == list(range(0, 64, 2)) + list(range(1, 64, 2)) and list(ids[1]) == list(range(1, 64, 2)) + list(range(0, 64, 2))
    assert list(dists[:, 0]) == [0.0] * 32 + [float(SI.EXTREME_MAX)] * 32 and list(matched) == [64, 64]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_the_tie_group_spans_rank_k(kind):
    ix, q, tied = SI.ties(kind)
    assert ix.N == SI.TIE_N and len(tied) == 50
    d = SR.distances(ix, q)
    # the copies straddle the 32-point tiles, the 128- and 256-point rounds' neighbours and the last ids
    assert {31, 32}.issubset(tied) and {63, 64}.issubset(tied) and {127, 128}.issubset(tied) and {159, 160}.issubset(tied) and {0, 199}.issubset(tied)
    for i in range(q.shape[0]):
        group = d[i, tied.astype(np.int64)]
        assert len(set(group.view(np.uint32).tolist())) == 1, "the copies are not at one distance"
        others = np.delete(d[i], tied.astype(np.int64))
        assert float(others.min()) > float(group[0]), "a point outside the group is as near as the copies"
    for k in (1, 10, 49):
        ids, dists, _ = SR.answer(d, k)
        assert all(list(ids[i]) == list(tied[:k]) for i in range(q.shape[0])), "the lowest ids of the tie group win"
        ids1, dists1, _ = SR.answer(d, k + 1)
        assert np.array_equal(dists1[k].view(np.uint32), dists[k - 1].view(np.uint32)), "rank k + 1 is still inside the group"


@pytest.mark.parametrize("name", SI.FIXTURES)
def test_excluding_the_true_ranks_changes_every_answer(request, name):
    ix, q = _fixture(request, name)
    d = SR.distances(ix, q)
    x = SI.excl_ranks(d)
    plain = SR.answer(d, 10)
    cut = SR.answer(d, 10, excluded=x)
    assert 5 <= len(x) <= 5 * q.shape[0]
    for i in range(q.shape[0]):
        assert not set(plain[0][i][:5].tolist()) & set(cut[0][i].tolist())
        assert not np.array_equal(plain[0][i], cut[0][i])
    assert (cut[2] == ix.N - len(x)).all() and (plain[2] == ix.N).all()
    few = SR.answer(d, 10, excluded=SI.excl_all_but(ix.N))
    assert (few[2] == 3).all() and (few[0][:, 3:] == SR.PAD_ID).all() and (few[1][3:] == SR.BIG_DIST).all() and (few[0][:, :3] != SR.PAD_ID).all()
    edges = SI.excl_edges(ix.N)
    assert list(edges) == [0, 31, 32, ix.N - 1]


@pytest.mark.parametrize("table,batch", SI.LABEL_CASES)
def test_label_cases_reach_their_edges(request, table, batch):
    ix, q = _fixture(request, "small_u8")
    Q = min(q.shape[0], 32)
    d = SR.distances(ix, q)[:Q]
    lab, a, b = SI.label_case(table, batch, ix, Q, d)
    ids, dists, matched = SR.answer(d, 10, labels=lab, any_=a, all_=b)
    if table == "nobody":
        assert (matched == 0).all() and (ids == SR.PAD_ID).all() and (dists == SR.BIG_DIST).all()
    elif table == "one_node":
        assert (matched >= 1).all() and np.array_equal(ids[:, 0], np.argmin(d, axis=1).astype(np.uint64))
    elif batch == "mixed":
        assert (matched[0::3] == ix.N).all() and (matched[1::3] < ix.N // 4).all() and (matched[1::3] > 0).all()
    elif table == "edges":
        assert (matched == len({0, 31, 32, ix.N - 1, int(ix.medoid)})).all()
    else:
        assert (matched > 0).all() and (matched < ix.N).all()
    for i in range(Q):                                                     # every returned id matches its query's filter
        got = ids[i][ids[i] != SR.PAD_ID].astype(np.int64)
        w = lab[got]
        assert ((a[i] == 0) | ((w & a[i]) != 0)).all() and ((w & b[i]) == b[i]).all()


def test_prefixes_and_padding():
    ix, q = SI.small("u8_32")
    d = SR.distances(ix, q)
    for n in SI.N_PREFIXES:
        ids, dists, matched = SR.answer(d, 100, n_nodes=n)
        m = min(n, 100)
        assert (matched == n).all() and (ids[:, :m] < n).all() and (ids[:, m:] == SR.PAD_ID).all() and (dists[m:] == SR.BIG_DIST).all()
