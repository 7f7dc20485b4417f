"""The query-resident search kernel of the LUT path (option "search" = 1 on an index with psz == 0; search_lut_kernel of
csrc/bang_search_lut.hip) against oracle.Oracle.search, which is itself the LUT arithmetic: ids, distance BITS and the four per-query counters
(iterations, candidates, distance evaluations, ids fetched).  Natural LUT layouts (chunks wider than 8 dimensions), the sum tails (m < 8,
m % 8 != 0), code rows that are not dword-aligned, pq = 1 forced on the fixtures, the edge inputs of tests/edge_inputs.py, batch and launch
shapes, MIPS, and the configurations that keep the loop they had."""
import numpy as np
import pytest

import edge_inputs as E
import highdim_inputs as H

pytestmark = pytest.mark.gpu

FIXTURES = ("small_u8", "small_i8", "small_f32", "small_deep")
TIE_FIXTURES = ("small_u8", "small_i8", "small_f32")
_REF = {}


def _oracle(key, ix, q, k, L, mips=False):
    """Oracle.search(..., with_stats=True), computed once per (input, k, L)."""
    from oracle import oracle as O
    if (key, k, L, mips) not in _REF:
        _REF[(key, k, L, mips)] = O.Oracle(ix).search(q, k, L, mips=mips, with_stats=True)
    return _REF[(key, k, L, mips)]


def _engine(ix, **opts):
    import bang_amd
    opts.setdefault("graph", bang_amd.GRAPH_DEVICE)
    opts.setdefault("search", 1)
    e = bang_amd.Engine(ix.dtype, **opts)
    e.load_index(ix)
    return e


def _run(e, q, k, L, distfn=0):
    e.set_searchparams(k, L, distfn)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    return ids, d, e.query_counters(q.shape[0])


def _assert_same(got, want):
    ids, d, st = got
    ids_r, d_r, st_r = want
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
    assert np.array_equal(st, st_r)                       # iterations, candidates, dist_evals, fetched


def _assert_lut_kernel(e):
    s = e.stats()
    assert s["search_kernel"] == 1 and s["persistent"] == 1 and s["front_launches"] == 1 and s["rerank_fused"] == 0
    assert s["lanes"] == 1


def _ks(L):
    return sorted({1, min(10, L), L})


def _check(e, key, ix, q, L, ks=None):
    for k in (_ks(L) if ks is None else ks):
        _assert_same(_run(e, q, k, L), _oracle(key, ix, q, k, L))
        _assert_lut_kernel(e)
        e.free()


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("gist_like", "mnist_like", "i8_1024", "f32_260"))
def test_natural_lut_layouts(name):
    """m = 120; m = 98 (m % 8 = 2); m = 64 with 16-dimension chunks; m = 65 (code rows not dword-aligned).  Fails without the kernel: these
    layouts then run the launch-per-iteration loop and report search_kernel == 0."""
    ix, q = H.get(name)
    with _engine(ix) as e:
        for L in (10, 37, 152):
            _check(e, name, ix, q, L, ks=(10,))


@pytest.mark.parametrize("N,D,dtype,R,m,Q", [(600, 90, "uint8", 64, 5, 3),       # m = 5 < 8: the tail alone (tests/test_gpu_random_configs.py)
                                              (500, 130, "uint8", 32, 13, 5)],    # m = 13: a group of eight and a tail of five; 10-dimension chunks, rows not dword-aligned
                         ids=["m5", "m13"])
def test_sum_tails(N, D, dtype, R, m, Q):
    from bang_amd import synth
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=5, n_clusters=8, seed=1000 + N + D, pq_iters=2)
    with _engine(ix) as e:
        for L in (5, 25):
            _check(e, ("tails", m), ix, q, L, ks=(5,))


@pytest.mark.parametrize("fixture", FIXTURES)
def test_forced_lut_path_on_the_fixtures(fixture, request):
    """pq = 1 on layouts that would get an LDS table (m = 70, 16, 32, 74); search = 0 -- the launch-per-iteration loop -- returns the same bits."""
    ix, q = request.getfixturevalue(fixture)[:2]
    with _engine(ix, pq=1) as e, _engine(ix, pq=1, search=0) as e0:
        for L in (10, 64, 512):
            want = _oracle(fixture, ix, q, 10, L)
            _assert_same(_run(e, q, 10, L), want)
            _assert_lut_kernel(e)
            e.free()
            ids0, d0, st0 = _run(e0, q, 10, L)
            assert np.array_equal(ids0, want[0]) and np.array_equal(d0.view(np.uint32), want[1].view(np.uint32))
            assert np.array_equal(st0[:, 1:], want[2][:, 1:])            # (the loop reports no per-query iterations)
            assert e0.stats()["search_kernel"] == 0
            e0.free()


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed_list_of_65(variant, dtype, D):
    ix, q = E.seed65(dtype, variant, D)
    with _engine(ix, pq=1) as e:
        for L in (4, 10, 37):
            _check(e, ("seed65", variant, dtype, D), ix, q, L)


@pytest.mark.parametrize("L", (10, 37))
def test_chain_runs_to_the_iteration_cap(L):
    ix, q = E.chain()
    cap = L + 49
    with _engine(ix, pq=1) as e:
        for k in _ks(L):
            got = _run(e, q, k, L)
            _assert_same(got, _oracle("chain", ix, q, k, L))
            assert got[2].tolist() == [[cap, cap + 1, cap + 1, cap + 1]]
            c_ids, c_cnt = e.candidate_log(1, L)
            assert int(c_cnt[0]) == L + 50 and c_ids[0].tolist() == list(range(L + 50))
            _assert_lut_kernel(e)
            e.free()


def test_short_worklist_is_padded():
    ix, q = E.short_worklist()
    with _engine(ix, pq=1) as e:
        _check(e, "short_worklist", ix, q, 16)
        _check(e, "short_worklist", ix, q, 152, ks=(100, 152))


@pytest.mark.parametrize("name", TIE_FIXTURES)
def test_tie_heavy_vectors_and_pivots(name, request):
    ix, q = E.tie_heavy(*request.getfixturevalue(name)[:2])
    with _engine(ix, pq=1) as e:
        for L in (10, 37):
            _check(e, ("tie_heavy", name), ix, q, L)
        if name == "small_u8":
            _check(e, ("tie_heavy4", name), ix, q[:4], 512, ks=(512,))


# ---------------------------------------------------------------------------------------------------------------------
# batch and launch shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_wgs", ("0", "2"))
def test_batch_sizes(small_u8, max_wgs, monkeypatch):
    ix, q = small_u8[:2]
    k, L = 10, 37
    qq = np.ascontiguousarray(np.tile(q, (11, 1))[:700])
    want = _oracle("small_u8x700", ix, qq, k, L)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", max_wgs)
    with _engine(ix, pq=1) as e:
        for Q in (1, 2, 63, 700):
            _assert_same(_run(e, qq[:Q], k, L), (want[0][:Q], np.ascontiguousarray(want[1][:, :Q]), want[2][:Q]))
            _assert_lut_kernel(e)
            e.free()


def test_one_wave_runs_every_query(small_u8, monkeypatch):
    ix, q = small_u8[:2]
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix, pq=1) as e:
        _assert_same(_run(e, q, 10, 37), _oracle("small_u8", ix, q, 10, 37))
        assert e.stats()["workgroups"] >= 1
        e.free()


def test_requery_and_realloc_on_one_engine(small_u8):
    ix, q = small_u8[:2]
    Q = q.shape[0]
    with _engine(ix, pq=1) as e:
        want = _oracle("small_u8", ix, q, 10, 37)
        _assert_same(_run(e, q, 10, 37), want)
        e.init(Q)                                              # init + query a second time on the same allocation
        ids, d = e.query(q)
        _assert_same((ids, d, e.query_counters(Q)), want)
        e.free()
        _assert_same(_run(e, q, 10, 64), _oracle("small_u8", ix, q, 10, 64))     # free, then alloc at another L
        _assert_lut_kernel(e)
        e.free()


def test_mips(small_f32):
    """MIPS: queries carry D - 1 coordinates (bang_search.cu:1099-1113); K1 builds the table, the re-rank launch handles the padding."""
    import bang_amd
    ix, q = small_f32[:2]
    q1 = np.ascontiguousarray(q[:, :-1])
    with _engine(ix, pq=1) as e:
        _assert_same(_run(e, q1, 10, 40, bang_amd.DIST_MIPS), _oracle("small_f32", ix, q1, 10, 40, mips=True))
        _assert_lut_kernel(e)
        e.free()


# ---------------------------------------------------------------------------------------------------------------------
# what does not change
# ---------------------------------------------------------------------------------------------------------------------
def test_default_search_option_keeps_the_loop(small_u8):
    import bang_amd
    ix, q = small_u8[:2]
    want = _oracle("small_u8", ix, q, 10, 37)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, pq=1) as e:
        e.load_index(ix)
        ids, d, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, want[0]) and np.array_equal(d.view(np.uint32), want[1].view(np.uint32))
        assert e.stats()["search_kernel"] == 0
        e.free()


def test_host_graph_keeps_the_loop(small_u8):
    import bang_amd
    ix, q = small_u8[:2]
    want = _oracle("small_u8", ix, q, 10, 37)
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pq=1) as e:
        ids, d, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, want[0]) and np.array_equal(d.view(np.uint32), want[1].view(np.uint32))
        assert e.stats()["search_kernel"] == 0
        e.free()


def test_inmemory_semantics_stay_refused_on_the_lut_path(small_u8):
    import bang_amd
    ix, q = small_u8[:2]
    with _engine(ix, pq=1, semantics=bang_amd.SEMANTICS_INMEMORY) as e:
        e.set_searchparams(10, 37)
        with pytest.raises(bang_amd.BangError, match="semantics"):
            e.alloc(q.shape[0])
