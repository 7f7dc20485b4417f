"""The beam form of the exact-distance search (options distance = 1, beam = W; csrc/bang_search_beam.hip) against its CPU reference
(tests/beam_reference.py), bit for bit: ids, distance bits, the four per-query counters and the candidate log -- with the graph in HBM and
with the rows pulled from host RAM, on the fixtures, on the edge inputs of tests/beam_inputs.py (tests/test_beam_mode.py asserts without a
GPU that they reach their edges), in every launch shape, and the refusals.  beam = 1 is today's exact-distance walk."""
import ctypes as C

import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
from beam_reference import Reference

pytestmark = pytest.mark.gpu

FIXTURES = ("small_u8", "small_i8", "small_f32", "small_deep")
NQ = 32                                       # queries per fixture: the reference walks them one by one on the CPU
_REF = {}


def _reference(key, ix, q, L, W):
    """The reference at k = L (a smaller k is a prefix: edge_inputs.first_k), computed once and shared."""
    if (key, L, W) not in _REF:
        _REF[(key, L, W)] = Reference(ix).search(q, L, L, W)
    return _REF[(key, L, W)]


def _engine(ix, beam, pulled=False, **opts):
    import bang_amd
    if pulled:
        opts.setdefault("pull", 1)
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST if pulled else bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT, beam=beam, **opts)
    e.load_index(ix)
    return e


def _run(e, q, k, L, Q=None):
    Q = q.shape[0] if Q is None else Q
    e.set_searchparams(k, L)
    e.alloc(Q)
    e.init(q.shape[0])
    ids, d = e.query(q)
    log, cnt = e.candidate_log(q.shape[0], L)
    return ids, d, e.query_counters(q.shape[0]), log, cnt


def _assert_same(got, want, k=None):
    ids, d, st, log, cnt = got
    ids_r, d_r, st_r, log_r = want
    if k is not None:
        ids_r, d_r, st_r = E.first_k((ids_r, d_r, st_r), k)
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
    assert np.array_equal(st, st_r)                       # iterations, candidates, dist_evals, fetched
    assert np.array_equal(cnt, st_r[:, 1])
    for i in range(ids.shape[0]):                         # the candidate log, in expansion order
        assert np.array_equal(log[i, :cnt[i]], log_r[i, :cnt[i]]), i


def _assert_stats(s, pulled):
    assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["rerank_fused"] == 0, s
    assert s["graph_pull"] == (1 if pulled else 0), s


# ------------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("name", FIXTURES)
def test_graph_in_hbm_matches_the_reference(name, W, request):
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:NQ]
    with _engine(ix, W) as e:
        for L in (10, 37, 152):
            ref = _reference(name, ix, q, L, W)
            got = _run(e, q, 10, L)
            _assert_same(got, ref, k=10)
            _assert_stats(e.stats(), False)
            if L == 37:                                   # init + query again on the same allocation reproduces the first run
                e.init(q.shape[0])
                ids2, d2 = e.query(q)
                assert np.array_equal(ids2, got[0]) and np.array_equal(d2.view(np.uint32), got[1].view(np.uint32))
                assert np.array_equal(e.query_counters(q.shape[0]), got[2])
            e.free()


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("name", FIXTURES)
def test_pulled_rows_match_the_reference(name, W, request, monkeypatch):
    """graph = host, pull = 1: every row over PCIe, then with the first third of the rows in their HBM copy."""
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:NQ]
    Q = q.shape[0]
    pulled = {}
    with _engine(ix, W, pulled=True) as e:
        for L in (10, 37, 152):
            _assert_same(_run(e, q, 10, L), _reference(name, ix, q, L, W), k=10)
            s = e.stats()
            _assert_stats(s, True)
            assert s["rows_in_hbm"] == 0 and s["pulled_bytes"] > 0, s
            pulled[L] = s["pulled_bytes"]
            e.free()
        e.unload()
    monkeypatch.setenv("BANG_ROWS_HBM_MAX_ROWS", str(ix.N // 3))
    with _engine(ix, W, pulled=True, rows_hbm=64) as e:
        L = 37
        _assert_same(_run(e, q, 10, L), _reference(name, ix, q, L, W), k=10)
        s = e.stats()
        _assert_stats(s, True)
        assert s["rows_in_hbm"] == ix.N // 3 and 0 < s["pulled_bytes"] < pulled[L], s
        assert s["rows_from_own_hbm"] * 256 + s["pulled_bytes"] == pulled[L], s
        e.free()
        e.unload()


# ------------------------------------------------------------------------------------------------------------------------ edge inputs
@pytest.mark.parametrize("pulled", [False, True], ids=["hbm", "pulled"])
@pytest.mark.parametrize("name,dtype,D", BI.cases(), ids=lambda v: str(v))
def test_edge_inputs(name, dtype, D, pulled):
    ix, q, beams, Ls = BI.build(name, dtype, D)
    for W in beams:
        with _engine(ix, W, pulled=pulled) as e:
            for L in Ls:
                ref = _reference(("edge", name, dtype, D), ix, q, L, W)
                for k in sorted({1, min(10, L), L}):                                  # k = L, and k < L as a prefix
                    _assert_same(_run(e, q, k, L), ref, k=k)
                    e.free()
            e.unload()


# ------------------------------------------------------------------------------------------------------------------------ launch shapes
@pytest.mark.parametrize("pulled", [False, True], ids=["hbm", "pulled"])
@pytest.mark.parametrize("name,W", [("small_u8", 4), ("small_deep", 2), ("small_i8", 3)])
def test_launch_shape_does_not_change_results(name, W, pulled, request, monkeypatch):
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:NQ]
    k, L = 10, 37
    ref = _reference(name, ix, q, L, W)
    want = E.first_k(ref[:3], k)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")                    # one workgroup of one wave runs every query in turn
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix, W, pulled=pulled) as e:
        _assert_same(_run(e, q, k, L), ref, k=k)
        e.free()
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "2")                    # two workgroups of several waves; the rest from the hand-out counter
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "5")
    with _engine(ix, W, pulled=pulled) as e:
        _assert_same(_run(e, q, k, L), ref, k=k)
        e.free()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    with _engine(ix, W, pulled=pulled) as e:                          # batches of 1, 7 and all on one allocation
        e.set_searchparams(k, L)
        e.alloc(q.shape[0])
        for nb in (1, 7, q.shape[0]):
            e.init(nb)
            ids, d = e.query(q[:nb])
            assert np.array_equal(ids, want[0][:nb])
            assert np.array_equal(d.view(np.uint32), want[1][:, :nb].view(np.uint32))
            assert np.array_equal(e.query_counters(nb), want[2][:nb])
        e.free()


def test_longest_worklist(small_u8):
    """L = 512 with k = L, the whole worklist compared.  Four queries launch as four workgroups of one wave; sixteen waves' worklists and survivor
    arrays side by side in one workgroup's LDS run in tests/test_gpu_launch_shapes.py (test_beam_longest_worklist)."""
    ix, q = E.tie_heavy(*small_u8[:2], n_queries=4)
    with _engine(ix, 4) as e:
        _assert_same(_run(e, q, 512, 512), _reference(("tie_heavy", 4), ix, q, 512, 4))
        e.free()


@pytest.mark.parametrize("pulled", [False, True], ids=["hbm", "pulled"])
def test_results_into_device_buffers(small_f32, pulled):
    import torch
    ix, q, _, _ = small_f32
    q = q[:NQ]
    Q, k, L, W = q.shape[0], 10, 37, 3
    ids_r, d_r, _ = E.first_k(_reference("small_f32", ix, q, L, W)[:3], k)
    d_ids = torch.zeros((Q, k), dtype=torch.int64, device="cuda")
    d_d = torch.zeros((k, Q), dtype=torch.float32, device="cuda")
    with _engine(ix, W, pulled=pulled) as e:
        e.set_searchparams(k, L)
        e.alloc(Q)
        e.init(Q)
        e.query_dev(q, d_ids.data_ptr(), d_d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), ids_r)
        assert np.array_equal(d_d.cpu().numpy().view(np.uint32), d_r.view(np.uint32))
        e.free()


# ------------------------------------------------------------------------------------------------------------------------ beam = 1
@pytest.mark.parametrize("pulled", [False, True], ids=["hbm", "pulled"])
@pytest.mark.parametrize("name", ["small_u8", "small_deep"])
def test_beam_one_is_todays_walk(name, pulled, request):
    from exact_reference import Reference as Exact
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:NQ]
    ids_r, d_r, st_r = Exact(ix).search(q, 10, 37, "exact")
    with _engine(ix, 1, pulled=pulled) as e:
        ids, d, st, _, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, ids_r) and np.array_equal(d.view(np.uint32), d_r.view(np.uint32)) and np.array_equal(st, st_r)
        e.free()


@pytest.mark.parametrize("W", [1, 4])
def test_kernel_level_launch(small_i8, W):
    """bang_k_search_exact_beam called directly (graph entries in HBM): beam = 1 -- the post-merge walk, which the engine never launches -- and 4."""
    import bang_amd
    from bang_amd import binding as B
    ix, q, _, _ = small_i8
    q = np.ascontiguousarray(q[:16])
    Q, k, L = q.shape[0], 10, 37
    ids_r, d_r, st_r, log_r = Reference(ix).search(q, k, L, W)
    lib = bang_amd.lib()
    adj = ix.adjacency()[ix.medoid][: int(ix.degrees()[ix.medoid])]
    seed = np.zeros(2 + 65, dtype=np.uint32)
    seed[0], seed[1] = 1 + len(adj), ix.medoid
    seed[2:2 + len(adj)] = adj
    buf = dict(seed=B.DeviceBuffer.from_numpy(seed), graph=B.DeviceBuffer.from_numpy(ix.graph, slack=256), q=B.DeviceBuffer.from_numpy(q, slack=16),
               bloom=B.DeviceBuffer(Q * B.BF_WORDS * 4), cand=B.DeviceBuffer(Q * (L + 50) * 4), cnt=B.DeviceBuffer(Q * 4), qstats=B.DeviceBuffer(Q * 8),
               iters=B.DeviceBuffer(Q * 4), ctl=B.DeviceBuffer(64), ids=B.DeviceBuffer(Q * k * 8), dists=B.DeviceBuffer(Q * k * 4))
    sp = B.SearchParams()
    sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter = Q, ix.R, L, ix.medoid, L + 49
    sp.d_seed, sp.d_graph, sp.entry_len, sp.vec_bytes, sp.n_nodes = buf["seed"].ptr, buf["graph"].ptr, ix.entry_len, ix.D, ix.N
    sp.d_bloom, sp.d_cand_ids, sp.d_cand_cnt, sp.d_qstats, sp.d_qiters = buf["bloom"].ptr, buf["cand"].ptr, buf["cnt"].ptr, buf["qstats"].ptr, buf["iters"].ptr
    sp.d_next_query, sp.d_abort = buf["ctl"].ptr, buf["ctl"].ptr + 4
    sp.rr_queries, sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = buf["q"].ptr, B.DTYPE_CODE[ix.dtype], ix.D, k, 0, Q
    sp.rr_ids_out, sp.rr_dists_out = buf["ids"].ptr, buf["dists"].ptr
    f = lib.bang_k_search_exact_beam
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    f.restype = C.c_int
    assert f(C.byref(sp), W, None) == 0, lib.bang_last_error().decode()
    B.sync()
    assert np.array_equal(buf["ids"].download(np.uint64, (Q, k)), ids_r)
    assert np.array_equal(buf["dists"].download(np.uint32, (k, Q)), d_r.view(np.uint32))
    cnt = buf["cnt"].download(np.uint32, (Q,))
    log = buf["cand"].download(np.uint32, (Q, L + 50))
    qs = buf["qstats"].download(np.uint32, (Q, 2))
    assert np.array_equal(buf["iters"].download(np.uint32, (Q,)), st_r[:, 0]) and np.array_equal(cnt, st_r[:, 1])
    assert np.array_equal(qs[:, 0], st_r[:, 2]) and np.array_equal(qs[:, 1], st_r[:, 3])
    for i in range(Q):
        assert np.array_equal(log[i, :cnt[i]], log_r[i, :cnt[i]])
    assert int(buf["ctl"].download(np.uint32, (2,))[1]) == 0                         # no id out of range


# ------------------------------------------------------------------------------------------------------------------------ the guard
def test_overwritten_rows_are_reported_not_followed(small_u8, tmp_path, monkeypatch):
    """Pulled rows overwritten behind the engine's back (a well-formed row whose first id is out of range): the id is compared, never turned
    into an address; the batch ends with an error naming the cause, and with the rows back the engine answers correctly again."""
    import bang_amd
    monkeypatch.setenv("BANG_PULL_ROWS_DIR", str(tmp_path))
    ix, q, _, _ = small_u8
    q = q[:NQ]
    k, L, W = 10, 37, 2
    ref = _reference("small_u8", ix, q, L, W)
    path = tmp_path / "index_pull_rows.bin"
    with _engine(ix, W, pulled=True) as e:
        _assert_same(_run(e, q, k, L), ref, k=k)
        rows = np.memmap(path, np.uint32, "r+", shape=(ix.N, 64))
        saved = np.array(rows[:, 0])
        rows[:, 0] = np.uint32(ix.N + 7)
        rows.flush()
        e.init(q.shape[0])
        with pytest.raises(bang_amd.BangError, match="out of range"):
            e.query(q)
        rows[:, 0] = saved
        rows.flush()
        del rows
        e.init(q.shape[0])
        ids, d = e.query(q)
        ids_r, d_r, _ = E.first_k(ref[:3], k)
        assert np.array_equal(ids, ids_r) and np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
        e.free()
        e.unload()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_unsupported_configurations_are_refused(small_u8, small_f32):
    import bang_amd
    import highdim_inputs as H
    ix, q, _, _ = small_u8

    def refused(ix_, q_, **opts):
        e = bang_amd.Engine(ix_.dtype, beam=2, **opts)
        try:
            e.load_index(ix_)
            e.set_searchparams(10, 37)
            with pytest.raises(bang_amd.BangError, match="beam"):
                e.alloc(q_.shape[0])
        finally:
            e.close()

    refused(ix, q, graph=bang_amd.GRAPH_DEVICE)                                                        # distance = 0
    refused(ix, q, graph=bang_amd.GRAPH_HOST, pull=1)
    refused(ix, q, graph=bang_amd.GRAPH_DEVICE, semantics=bang_amd.SEMANTICS_INMEMORY)
    refused(ix, q, graph=bang_amd.GRAPH_DEVICE, distance=1, semantics=bang_amd.SEMANTICS_INMEMORY)
    refused(ix, q, graph=bang_amd.GRAPH_HOST, pull=1, distance=1, semantics=bang_amd.SEMANTICS_INMEMORY)
    ixf, qf, _, _ = small_f32
    refused(ixf, qf, graph=bang_amd.GRAPH_HOST, pull=1, distance=1, vectors_fp16=1)                    # an fp16 vector table
    ixw, qw = H.get("u8_48")                                                                           # 8-bit, D / 16 = 3: a wide layout
    refused(ixw, qw, graph=bang_amd.GRAPH_DEVICE, distance=1)
    refused(ixw, qw, graph=bang_amd.GRAPH_HOST, pull=1, distance=1)
    for bad in (0, 5):
        with bang_amd.Engine(ix.dtype) as e:
            with pytest.raises(bang_amd.BangError):
                e.set_option("beam", bad)
