"""BANG_Inmemory search semantics on the GPU (option "semantics" = 1, search_inmem_kernel of csrc/bang_search.hip): bit parity with the CPU
reference composed from the oracle's stages (tests/inmemory_reference.py), tie-heavy codes, the iteration cap, launch-shape independence,
device-buffer results, base semantics after an inmemory run, the refusals and the CLI."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from inmemory_reference import Reference, chain_index, medoid_tie_index, medoid_tie_variant

pytestmark = pytest.mark.gpu

FIXTURES = ("small_u8", "small_f32", "small_i8", "small_deep")
_REF = {}


def _reference(name, ix, q, k, L, mode="inmemory"):
    key = (name, k, L, mode)
    if key not in _REF:
        _REF[key] = Reference(ix).search(q, k, L, mode)
    return _REF[key]


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


@pytest.mark.timeout(400, method="thread")
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("fuse", [1, 0])
def test_inmemory_matches_the_reference_bit_for_bit(name, fuse, request):
    ix, q, _, _ = request.getfixturevalue(name)
    with _engine(ix, fuse_rerank=fuse) as e:
        for k, L in ((10, 10), (10, 37), (10, 152)):
            _assert_same(_run(e, q, k, L), _reference(name, ix, q, k, L))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["rerank_fused"] == fuse
            e.free()


def _tie_heavy(ix):
    """small_u8 with every third node's code row replaced by that of its first neighbour: exact PQ ties between neighbours."""
    adj, deg = ix.adjacency(), ix.degrees()
    codes = ix.codes.copy()
    for i in range(0, ix.N, 3):
        if deg[i] > 0:
            codes[i] = ix.codes[adj[i][0]]
    return dataclasses.replace(ix, codes=codes)


@pytest.mark.timeout(400, method="thread")
def test_tie_heavy_codes(small_u8):
    ix, q, _, _ = small_u8
    ix2 = _tie_heavy(ix)
    for L in (10, 37):
        base = _reference("tie_u8", ix2, q, 10, L, "base")
        inm = _reference("tie_u8", ix2, q, 10, L, "inmemory")
        assert (base[2] != inm[2]).any(axis=1).sum() > 0         # the two walks differ on these codes
        with _engine(ix2) as e:
            _assert_same(_run(e, q, 10, L), inm)
            e.free()


@pytest.mark.timeout(300, method="thread")
def test_medoid_tying_the_best_neighbour(small_u8):
    """Iteration 1 with the medoid sorted in front of an equal best neighbour: the parent is marked at its own slot, not the medoid's."""
    ix, q = medoid_tie_index()
    want = Reference(ix).search(q, 5, 10, "inmemory")
    assert want[2][0].tolist() == [5, 5, 5, 5]
    with _engine(ix) as e:
        _assert_same(_run(e, q, 5, 10), want)
        c_ids, c_cnt = e.candidate_log(1, 10, 120)
        assert c_ids[0][:int(c_cnt[0])].tolist() == [0, 1, 3, 2, 4]
        e.free()
    ix2, q2, _ = medoid_tie_variant(*small_u8[:2])
    with _engine(ix2) as e:
        for L in (10, 37):
            _assert_same(_run(e, q2, 10, L), _reference("medoid_tie_u8", ix2, q2, 10, L))
            e.free()


@pytest.mark.timeout(300, method="thread")
def test_chain_graph_runs_to_the_cap():
    import bang_amd
    ix, q = chain_index()
    for L in (10, 37):
        want = Reference(ix).search(q, 10, L, "inmemory")
        assert want[2][0].tolist() == [L + 119, L + 120, L + 120, L + 120]
        with _engine(ix) as e:
            got = _run(e, q, 10, L)
            _assert_same(got, want)
            c_ids, c_cnt = e.candidate_log(1, L, 120)                # the log holds L + 120 entries: every node of the chain up to the cap
            assert int(c_cnt[0]) == L + 120 and c_ids[0].tolist() == list(range(L + 120))
            with pytest.raises(bang_amd.BangError, match=r"L \+ 120"):
                e.candidate_log(1, L)
            e.free()


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", ["small_u8", "small_deep"])
def test_launch_shape_does_not_change_results(name, request, monkeypatch):
    ix, q, _, _ = request.getfixturevalue(name)
    k, L = 10, 37
    ref = _reference(name, ix, q, k, L)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")                 # one wave runs every query in turn
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix) as e:
        _assert_same(_run(e, q, k, L), ref)
        e.free()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    with _engine(ix) as e:                                         # batch sizes 1, 7 and all, on one allocation
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
def test_base_semantics_unchanged_after_an_inmemory_run(small_u8):
    import bang_amd
    from oracle import oracle as O
    ix, q, _, _ = small_u8
    ids_o, d_o, st_o = O.Oracle(ix).search(q, 10, 37, with_stats=True)
    with _engine(ix) as e:
        _assert_same(_run(e, q, 10, 37), _reference("small_u8", ix, q, 10, 37))
        e.free()
        e.set_option("semantics", bang_amd.SEMANTICS_BASE)          # the same engine, the same index
        ids, d, st = _run(e, q, 10, 37)
        assert np.array_equal(ids, ids_o) and np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
        assert np.array_equal(st, st_o)                                 # all four columns: the iteration count shows the cap (L + 49)
        e.free()


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("word,mode", [("inmemory", "inmemory"), ("base", "base")])
def test_environment_selects_the_semantics(small_i8, monkeypatch, word, mode):
    import bang_amd
    ix, q, _, _ = small_i8
    monkeypatch.setenv("BANG_SEMANTICS", word)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
        e.load_index(ix)
        ids, d, st = _run(e, q, 10, 37)
        want = _reference("small_i8", ix, q, 10, 37, mode)
        assert np.array_equal(ids, want[0]) and np.array_equal(d.view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(st, want[2])                              # all four columns, the iteration count included
        e.free()


@pytest.mark.timeout(300, method="thread")
def test_unsupported_configurations_are_refused(small_u8):
    import bang_amd
    ix, q, _, _ = small_u8

    def refused(mips=False, **opts):
        e = bang_amd.Engine(ix.dtype, semantics=bang_amd.SEMANTICS_INMEMORY, **opts)
        try:
            e.load_index(ix)
            e.set_searchparams(10, 37, bang_amd.DIST_MIPS if mips else bang_amd.DIST_L2)
            with pytest.raises(bang_amd.BangError, match="semantics"):
                e.alloc(q.shape[0])
                e.init(q.shape[0])
                e.query(q[:, :-1] if mips else q)
        finally:
            e.close()

    refused(graph=bang_amd.GRAPH_HOST)
    refused(graph=bang_amd.GRAPH_DEVICE, search=0)
    refused(graph=bang_amd.GRAPH_DEVICE, persistent=0)
    refused(graph=bang_amd.GRAPH_DEVICE, pq=1)
    refused(mips=True, graph=bang_amd.GRAPH_DEVICE)
    refused(graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT)


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_SEMANTICS=inmemory BANG_GRAPH=device bang_search (interactive L) prints the usual table; its recall at each L is the reference's."""
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
    env = dict(os.environ, BANG_SEMANTICS="inmemory", BANG_GRAPH="device")
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
