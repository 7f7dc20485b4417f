"""Exact-distance search with the adjacency rows pulled by the kernel (options graph = host, pull = 1, distance = 1; the pulled-rows instances
of csrc/bang_search_exact.hip): the rows come from pinned host memory, from the HBM copy of the first rows or from a slice table, the vectors
from the packed table in HBM.  The CPU reference (tests/exact_reference.py) reads the adjacency from the index and knows nothing of
placement, so every run here equals it bit for bit: ids, distance bits and the four per-query counters."""
import os
import subprocess

import numpy as np
import pytest

import edge_inputs as E
import highdim_inputs as H
from exact_reference import Reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("small_u8", "small_i8", "small_f32", "small_deep")
_REF = {}


def _reference(key, ix, q, k, L):
    if (key, k, L) not in _REF:
        _REF[(key, k, L)] = Reference(ix).search(q, k, L, "exact")
    return _REF[(key, k, L)]


def _engine(ix, graph=None, **opts):
    import bang_amd
    if graph is None:
        graph = bang_amd.GRAPH_HOST
    if graph == bang_amd.GRAPH_HOST:
        opts.setdefault("pull", 1)
    e = bang_amd.Engine(ix.dtype, graph=graph, distance=bang_amd.DISTANCE_EXACT, **opts)
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


def _assert_pulled_stats(s, Q):
    assert s["graph_pull"] == 1 and s["vectors_on_device"] == 1 and s["search_kernel"] == 1 and s["front_launches"] == 1, s
    assert s["rerank_fused"] == 0 and s["walker_threads"] == 0, s


def _check(e, key, ix, q, k, L):
    """One pulled run against the reference; every row over PCIe."""
    _assert_same(_run(e, q, k, L), _reference(key, ix, q, k, L))
    s = e.stats()
    _assert_pulled_stats(s, q.shape[0])
    assert s["pulled_bytes"] == 256 * (int(s["candidates"]) - q.shape[0]), s
    e.free()


# ------------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", FIXTURES)
def test_pulled_form_matches_the_reference_and_the_graph_in_hbm(name, request):
    import bang_amd
    ix, q, _, _ = request.getfixturevalue(name)
    Q = q.shape[0]
    cases = ((10, 10), (10, 37), (10, 152))
    in_hbm = {}
    with _engine(ix, graph=bang_amd.GRAPH_DEVICE) as e:
        for k, L in cases:
            in_hbm[(k, L)] = _run(e, q, k, L)
            e.free()
    with _engine(ix) as e:
        for k, L in cases:
            got = _run(e, q, k, L)
            _assert_same(got, _reference(name, ix, q, k, L))
            _assert_same(got, in_hbm[(k, L)])
            s = e.stats()
            _assert_pulled_stats(s, Q)
            assert s["rows_in_hbm"] == 0 and s["pulled_bytes"] == 256 * (int(s["candidates"]) - Q), s
            if L == 37:                                   # a second init + query on the same allocation reproduces the first run
                e.init(Q)
                ids2, d2 = e.query(q)
                assert np.array_equal(ids2, got[0]) and np.array_equal(d2.view(np.uint32), got[1].view(np.uint32))
                assert np.array_equal(e.query_counters(Q), got[2])
            e.free()


# ------------------------------------------------------------------------------------------------------------------------ row sources
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_rows_partly_and_wholly_in_hbm(name, request, monkeypatch):
    """Option rows_hbm: the rows of the first nodes are read from their HBM copy, the rest over PCIe; pulled_bytes counts the PCIe rows."""
    ix, q, _, _ = request.getfixturevalue(name)
    Q, k, L = q.shape[0], 10, 37
    ref = _reference(name, ix, q, k, L)

    def run(**opts):
        with _engine(ix, **opts) as e:
            _assert_same(_run(e, q, k, L), ref)
            s = e.stats()
            _assert_pulled_stats(s, Q)
            e.free()
            e.unload()
        return s
    base = run()
    assert base["rows_in_hbm"] == 0 and base["pulled_bytes"] == 256 * (int(base["candidates"]) - Q)
    monkeypatch.setenv("BANG_ROWS_HBM_MAX_ROWS", str(ix.N // 3))
    part = run(rows_hbm=64)
    assert part["rows_in_hbm"] == ix.N // 3 and 0 < part["pulled_bytes"] < base["pulled_bytes"], part
    assert part["rows_from_own_hbm"] * 256 + part["pulled_bytes"] == base["pulled_bytes"], part
    monkeypatch.delenv("BANG_ROWS_HBM_MAX_ROWS")
    full = run(rows_hbm=64)
    assert full["rows_in_hbm"] == ix.N and full["pulled_bytes"] == 0, full


@pytest.mark.timeout(300, method="thread")
def test_slice_table_with_an_absent_slot(small_u8):
    """A table of two slots in one process: slot 0 is this engine's own HBM slice (rows [0, n)), slot 1 is absent (a zero base: host rows) and
    the last third of the nodes lies beyond the table (host rows as well)."""
    ix, q, _, _ = small_u8
    Q, k, L = q.shape[0], 10, 37
    n = ix.N // 3
    with _engine(ix) as e:
        e.rows_slice(0, n)
        e.rows_import(0, 2, n, None)
        _assert_same(_run(e, q, k, L), _reference("small_u8", ix, q, k, L))
        s = e.stats()
        _assert_pulled_stats(s, Q)
        assert s["rows_from_own_hbm"] > 0 and s["rows_from_peer"] == 0 and s["pulled_bytes"] > 0, s
        assert s["rows_from_own_hbm"] * 256 + s["pulled_bytes"] == 256 * (int(s["candidates"]) - Q), s
        c_ids, c_cnt = e.candidate_log(Q, L)
        own = sum(int((c_ids[i, 1:c_cnt[i]] < n).sum()) for i in range(Q))
        assert s["rows_from_own_hbm"] == own
        e.free()
        e.unload()


# ------------------------------------------------------------------------------------------------------------------------ wide instances
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name,L", [("gist_like", 37), ("mnist_like", 152), ("u8_48", 37)])
def test_wide_layouts(name, L):
    """The pulled wide instances: 960 floats, 784 bytes (D / 16 = 49) and D / 16 = 3."""
    ix, q = H.get(name)
    with _engine(ix) as e:
        _check(e, ("highdim", name), ix, q, 10, L)


# ------------------------------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("dtype,D", [("uint8", 128), ("int8", 64), ("float", 20)])
@pytest.mark.parametrize("name", sorted(E.TOYS))
def test_toy_graphs_and_rows_of_pads_only(name, dtype, D):
    """Distance ties; the leaves of these graphs have degree 0 -- a row of pads only -- and at L = 10 every walk expands one: it logs more
    candidates than there are nodes with a neighbour, and no node is expanded twice."""
    ix, q = E.toy_named(name, dtype, D)
    assert int(_reference(("toy", name, dtype, D), ix, q, 3, 10)[2][0][1]) > int((ix.degrees() > 0).sum())
    with _engine(ix) as e:
        for L in (3, 10):
            _check(e, ("toy", name, dtype, D), ix, q, 3, L)


@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed_list_of_65(variant, dtype, D):
    """The medoid has degree 64: the seed list holds 65 ids, the 65th best / tying the best / worse; every later row comes as a pull row."""
    ix, q = E.seed65(dtype, variant, D)
    assert int(ix.degrees()[0]) == 64
    with _engine(ix) as e:
        for L in (4, 10, 37):
            _check(e, ("seed65", variant, dtype, D), ix, q, 4, L)


@pytest.mark.parametrize("dtype,D", E.DEGREE64_LAYOUTS)
def test_expanded_node_of_degree_64(dtype, D):
    """Node 1 is the first parent and has exactly 64 neighbours: its 256-byte row holds no pad and all 64 lanes carry an id."""
    ix, q = E.degree64(dtype, D)
    assert int(ix.degrees()[1]) == 64
    with _engine(ix) as e:
        for L in (5, 37):
            _check(e, ("deg64", dtype, D), ix, q, 5, L)
            ref = _reference(("deg64", dtype, D), ix, q, 5, L)
            assert int(ref[2][0][3]) >= 64 + 2                       # fetched: the seed list and the full row


@pytest.mark.parametrize("dtype,D", [("uint8", 128), ("float", 128)])
def test_chain_runs_to_the_cap(dtype, D):
    ix, q = E.chain(dtype, D)
    with _engine(ix) as e:
        for L in (10, 37):
            cap = L + 49
            ref = _reference(("chain", dtype, D), ix, q, 10, L)
            assert ref[2][0].tolist() == [cap, cap + 1, cap + 1, cap + 1]
            _check(e, ("chain", dtype, D), ix, q, 10, L)


@pytest.mark.parametrize("dtype,D", [("uint8", 128), ("int8", 64), ("float", 128)])
def test_short_worklist_is_padded(dtype, D):
    ix, q = E.short_worklist(dtype, D)
    ref = _reference(("short", dtype, D), ix, q, 10, 16)
    assert ref[0][0].tolist() == [1, 2, 0] + [int(E.ID_PAD)] * 7
    with _engine(ix) as e:
        _check(e, ("short", dtype, D), ix, q, 10, 16)


@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_tie_heavy_vectors(name, request):
    ix, q = E.tie_heavy(*request.getfixturevalue(name)[:2])
    assert E.ties_in_top(_reference(("tie_heavy", name), ix, q, 10, 37)[1], 10).any()
    with _engine(ix) as e:
        _check(e, ("tie_heavy", name), ix, q, 10, 37)


@pytest.mark.parametrize("shape", [s for s in E.SHAPES if s[3] < 64 and s[1] in (32, 20, 256)], ids=E.shape_id)
def test_degree_bound_below_64(shape):
    """R = 8 / 32: every row ends in at least 32 pads, and the kernel's clamp to R never cuts an id."""
    ix, q = E.shape_index(shape)
    assert ix.R < 64
    with _engine(ix) as e:
        _check(e, ("shape", shape), ix, q, 10, 37)


# ------------------------------------------------------------------------------------------------------------------------ launch shape
@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("name", ["small_u8", "small_deep"])
def test_launch_shape_does_not_change_results(name, request, monkeypatch):
    ix, q, _, _ = request.getfixturevalue(name)
    k, L = 10, 37
    ref = _reference(name, ix, q, k, L)
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")                    # one wave runs every query in turn
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    with _engine(ix) as e:
        _assert_same(_run(e, q, k, L), ref)
        e.free()
    monkeypatch.delenv("BANG_SEARCH_MAX_WGS")
    monkeypatch.delenv("BANG_SEARCH_MAX_WAVES")
    with _engine(ix) as e:                                            # batches of 1, 7 and all on one allocation
        e.set_searchparams(k, L)
        e.alloc(q.shape[0])
        for nb in (1, 7, q.shape[0]):
            e.init(nb)
            ids, d = e.query(q[:nb])
            assert np.array_equal(ids, ref[0][:nb])
            assert np.array_equal(d.view(np.uint32), ref[1][:, :nb].view(np.uint32))
            assert np.array_equal(e.query_counters(nb), ref[2][:nb])
        e.free()


# ------------------------------------------------------------------------------------------------------------------------ the guard
@pytest.mark.timeout(300, method="thread")
def test_overwritten_rows_are_reported_not_followed(small_u8, tmp_path, monkeypatch):
    """Rows overwritten behind the engine's back (an id out of range in column 0 of every row) end the batch with an error naming the cause;
    the id is never turned into an address.  Once the rows are back the engine answers correctly again."""
    import bang_amd
    monkeypatch.setenv("BANG_PULL_ROWS_DIR", str(tmp_path))
    ix, q, _, _ = small_u8
    k, L = 10, 37
    ref = _reference("small_u8", ix, q, k, L)
    path = tmp_path / "index_pull_rows.bin"
    with _engine(ix) as e:
        _assert_same(_run(e, q, k, L), ref)
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
        _assert_same((ids, d, e.query_counters(q.shape[0])), ref)
        e.free()
        e.unload()


# ------------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.timeout(300, method="thread")
def test_unsupported_configurations_are_refused(small_u8):
    import bang_amd
    from bang_amd import synth
    ix, q, _, _ = small_u8

    def refused(ix_, q_, mips=False, **opts):
        e = bang_amd.Engine(ix_.dtype, graph=bang_amd.GRAPH_HOST, distance=bang_amd.DISTANCE_EXACT, **opts)
        try:
            e.load_index(ix_)
            e.set_searchparams(10, 37, bang_amd.DIST_MIPS if mips else bang_amd.DIST_L2)
            with pytest.raises(bang_amd.BangError, match="distance"):
                e.alloc(q_.shape[0])
                e.init(q_.shape[0])
                e.query(q_[:, :-1] if mips else q_)
        finally:
            e.close()

    refused(ix, q)                                                    # pull left at auto: the pulled-rows form only when asked for
    refused(ix, q, pull=1, walker=1)
    refused(ix, q, pull=1, search=0)
    refused(ix, q, pull=1, persistent=0)
    refused(ix, q, mips=True, pull=1)
    refused(ix, q, pull=1, semantics=bang_amd.SEMANTICS_INMEMORY)
    ix8, q8, _, _ = synth.make_index(600, 40, "uint8", 32, 10, 8, K=10, n_clusters=8, seed=5, device="cpu", pq_iters=2)
    refused(ix8, q8, pull=1)                                          # 8-bit vectors with D % 16 != 0
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, distance=bang_amd.DISTANCE_EXACT, pull=1, vectors=0)
    try:
        with pytest.raises(bang_amd.BangError, match="pull"):         # no resident vectors: refused at load, as without distance = 1
            e.load_index(ix)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------ CLI
@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_DISTANCE=exact BANG_GRAPH=host BANG_PULL=1 bang_search prints the usual table; its recall at each L is the reference's."""
    import bang_amd
    from bang_amd import formats
    from oracle import oracle as O
    ix, q, gt_i, gt_d = small_i8
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    formats.write_truthset(str(tmp_path / "gt.bin"), gt_i, gt_d)
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    Ls = (10, 37)
    env = dict(os.environ, BANG_DISTANCE="exact", BANG_GRAPH="host", BANG_PULL="1")
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


# ------------------------------------------------------------------------------------------------------------------------ PQ unaffected
@pytest.mark.timeout(300, method="thread")
def test_pq_pull_mode_is_unaffected_after_an_exact_pulled_run(small_u8):
    import bang_amd
    from oracle import oracle as O
    ix, q, _, _ = small_u8
    with _engine(ix) as e:
        _run(e, q, 10, 37)
        e.free()
    ids_o, d_o = O.Oracle(ix).search(q, 10, 37)
    with bang_amd.Engine(ix.dtype, graph=0, pull=1) as e:
        e.load_index(ix)
        ids, d, _ = _run(e, q, 10, 37)
        assert np.array_equal(ids, ids_o) and np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
        s = e.stats()
        assert s["rerank_fused"] == 1 and s["graph_pull"] == 1
        e.free()
