"""The exact-distance search mode (option "distance" = 1) on the wide vector layouts -- D up to 1024, 8-bit vectors with any D / 16, 8-bit
distances past 2^24 (tests/highdim_inputs.py): bit parity with the CPU reference (tests/exact_reference.py) for every query of every input,
launch-shape independence, device-buffer results, the modes that ran before, and the refusals."""
import numpy as np
import pytest

import highdim_inputs as H
from exact_reference import Reference

pytestmark = pytest.mark.gpu

KL = ((10, 10), (10, 37), (10, 152))
_REF = {}


def _reference(name, k, L):
    key = (name, k, L)
    if key not in _REF:
        ix, q = H.get(name)
        _REF[key] = Reference(ix).search(q, k, L, "exact")
    return _REF[key]


def _engine(ix, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT, **opts)
    e.load_index(ix)
    return e


def _run(e, q, k, L):
    e.set_searchparams(k, L)
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


@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("name", H.NAMES)
def test_wide_layouts_match_the_reference_bit_for_bit(name):
    ix, q = H.get(name)
    with _engine(ix) as e:
        for k, L in KL:
            _assert_same(_run(e, q, k, L), _reference(name, k, L))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["rerank_fused"] == 0
            e.free()


@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("name", H.NAMES)
def test_launch_shape_does_not_change_results(name, monkeypatch):
    ix, q = H.get(name)
    k, L = 10, 37
    ref = _reference(name, k, L)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")        # one wave runs every query in turn
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix) as e:
        _assert_same(_run(e, q, k, L), ref)
        e.free()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    with _engine(ix) as e:                                # batches of 1, 7 and all on one allocation
        e.set_searchparams(k, L)
        e.alloc(q.shape[0])
        for nb in (1, 7, q.shape[0]):
            e.init(nb)
            ids, d = e.query(q[:nb])
            assert np.array_equal(ids, ref[0][:nb])
            assert np.array_equal(d.view(np.uint32), ref[1][:, :nb].view(np.uint32))
            assert np.array_equal(e.query_counters(nb), ref[2][:nb])
        e.free()


@pytest.mark.timeout(300, method="thread")
def test_results_into_device_buffers():
    import torch
    ix, q = H.get("gist_like")
    k, L = 10, 37
    ids_r, d_r, _ = _reference("gist_like", k, L)
    Q = q.shape[0]
    d_ids = torch.zeros((Q, k), dtype=torch.int64, device="cuda")
    d_d = torch.zeros((k, Q), dtype=torch.float32, device="cuda")
    with _engine(ix) as e:
        e.set_searchparams(k, L)
        e.alloc(Q)
        e.init(Q)
        e.query_dev(q, d_ids.data_ptr(), d_d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), ids_r)
        assert np.array_equal(d_d.cpu().numpy().view(np.uint32), d_r.view(np.uint32))
        e.free()


@pytest.mark.timeout(600, method="thread")
def test_other_modes_are_unaffected_after_a_wide_run(small_u8):
    import bang_amd
    from oracle import oracle as O
    ix, q = H.get("gist_like")
    with _engine(ix) as e:
        _run(e, q, 10, 37)
        e.free()
    # the narrow instances
    ix8, q8, _, _ = small_u8
    with _engine(ix8) as e:
        _assert_same(_run(e, q8, 10, 37), Reference(ix8).search(q8, 10, 37, "exact"))
        e.free()
    # the PQ walk on the wide index
    ids_o, d_o = O.Oracle(ix).search(q, 10, 37)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
        e.load_index(ix)
        ids, d, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, ids_o) and np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
        e.free()


@pytest.mark.timeout(300, method="thread")
def test_unsupported_configurations_are_refused():
    import bang_amd
    from bang_amd import synth

    def refused(ix_, q_, **opts):
        e = bang_amd.Engine(ix_.dtype, distance=bang_amd.DISTANCE_EXACT, **opts)
        try:
            e.load_index(ix_)
            e.set_searchparams(10, 37)
            with pytest.raises(bang_amd.BangError, match="distance"):
                e.alloc(q_.shape[0])
                e.init(q_.shape[0])
                e.query(q_)
        finally:
            e.close()

    ixf, qf, _, _ = synth.make_index(300, 1028, "float", 16, 257, 4, K=10, n_clusters=4, seed=6, device="cpu", pq_iters=1)
    refused(ixf, qf, graph=bang_amd.GRAPH_DEVICE)
    ix8, q8, _, _ = synth.make_index(600, 40, "uint8", 32, 10, 8, K=10, n_clusters=8, seed=5, device="cpu", pq_iters=2)
    refused(ix8, q8, graph=bang_amd.GRAPH_DEVICE)
    ix, q = H.get("gist_like")
    refused(ix, q, graph=bang_amd.GRAPH_HOST)
