"""Exact-distance search mode on the GPU (option "distance" = 1, csrc/bang_search_exact.hip): bit parity with the CPU reference composed from
the oracle's stages (tests/exact_reference.py), launch-shape independence, device-buffer results, refusals and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from exact_reference import Reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("small_u8", "small_f32", "small_i8", "small_deep")
_REF = {}


def _reference(name, ix, q, k, L):
    key = (name, k, L)
    if key not in _REF:
        _REF[key] = Reference(ix).search(q, k, L, "exact")
    return _REF[key]


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


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", FIXTURES)
def test_exact_mode_matches_the_reference_bit_for_bit(name, request):
    ix, q, _, _ = request.getfixturevalue(name)
    with _engine(ix) as e:
        for k, L in ((10, 10), (10, 37), (10, 152)):
            got = _run(e, q, k, L)
            _assert_same(got, _reference(name, ix, q, k, L))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["rerank_fused"] == 0
            if L == 37:                                   # a second init + query on the same allocation reproduces the first run
                e.init(q.shape[0])
                ids2, d2 = e.query(q)
                assert np.array_equal(ids2, got[0]) and np.array_equal(d2.view(np.uint32), got[1].view(np.uint32))
            e.free()


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", ["small_u8", "small_deep"])
def test_launch_shape_does_not_change_results(name, request, monkeypatch):
    ix, q, _, _ = request.getfixturevalue(name)
    k, L = 10, 37
    ref = _reference(name, ix, q, k, L)
    # one wave runs every query in turn (per-query state reset)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix) as e:
        _assert_same(_run(e, q, k, L), ref)
        e.free()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    # batch sizes 1, 7 and all, on one allocation
    with _engine(ix) as e:
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
def test_results_into_device_buffers(small_f32):
    import torch
    ix, q, _, _ = small_f32
    k, L = 10, 37
    ids_r, d_r, _ = _reference("small_f32", ix, q, k, L)
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


@pytest.mark.timeout(300, method="thread")
def test_pq_mode_is_unaffected_after_an_exact_run(small_u8):
    import bang_amd
    from oracle import oracle as O
    ix, q, _, _ = small_u8
    with _engine(ix) as e:
        _run(e, q, 10, 37)
        e.free()
    ids_o, d_o = O.Oracle(ix).search(q, 10, 37)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
        e.load_index(ix)
        ids, d, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, ids_o) and np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
        assert e.stats()["rerank_fused"] == 1
        e.free()


@pytest.mark.timeout(300, method="thread")
def test_unsupported_configurations_are_refused(small_u8, small_i8):
    import bang_amd
    from bang_amd import synth
    ix, q, _, _ = small_u8

    def refused(ix_, q_, mips=False, **opts):
        e = bang_amd.Engine(ix_.dtype, distance=bang_amd.DISTANCE_EXACT, **opts)
        try:
            e.load_index(ix_)
            e.set_searchparams(10, 37, bang_amd.DIST_MIPS if mips else bang_amd.DIST_L2)
            with pytest.raises(bang_amd.BangError, match="distance"):
                e.alloc(q_.shape[0])
                e.init(q_.shape[0])
                e.query(q_[:, :-1] if mips else q_)
        finally:
            e.close()

    refused(ix, q, graph=bang_amd.GRAPH_HOST)
    refused(ix, q, graph=bang_amd.GRAPH_DEVICE, search=0)
    refused(ix, q, graph=bang_amd.GRAPH_DEVICE, persistent=0)
    refused(ix, q, mips=True, graph=bang_amd.GRAPH_DEVICE)
    # a vector layout the kernel does not evaluate: 8-bit vectors with D % 16 != 0
    ix8, q8, _, _ = synth.make_index(600, 40, "uint8", 32, 10, 8, K=10, n_clusters=8, seed=5, device="cpu", pq_iters=2)
    refused(ix8, q8, graph=bang_amd.GRAPH_DEVICE)


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_DISTANCE=exact BANG_GRAPH=device bang_search (interactive L) prints the usual table; its recall at each L is the reference's."""
    import bang_amd
    from bang_amd import formats
    from oracle import oracle as O
    ix, q, gt_i, gt_d = small_i8
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    formats.write_truthset(str(tmp_path / "gt.bin"), gt_i, gt_d)
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    Ls = (10, 37, 152)
    env = dict(os.environ, BANG_DISTANCE="exact", BANG_GRAPH="device")
    out = subprocess.run([exe, prefix, str(tmp_path / "q.bin"), str(tmp_path / "gt.bin"), str(q.shape[0]), "10", "int8", "l2"],
                         input="".join(f"{L}\ny\n" for L in Ls[:-1]) + f"{Ls[-1]}\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split("\t") for l in out.stdout.splitlines() if l[:1].isdigit() and l.count("\t") == 3]
    assert "10-r@10" in out.stdout and sorted({int(r[0]) for r in rows}) == list(Ls)
    for L in Ls:
        ids, _, _ = _reference("small_i8", ix, q, 10, L)
        want = f"{float(np.float32(O.recall(gt_i, gt_d, ids, 10))):.2f}"
        got = [r[3].strip() for r in rows if int(r[0]) == L]
        assert len(got) == 5 and all(g == want for g in got), (L, got, want)
