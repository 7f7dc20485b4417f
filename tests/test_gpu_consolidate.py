"""Consolidation on a GPU (csrc/bang_consolidate.hip, bang_consolidate_e), bit for bit / byte for byte against tests/consolidate_reference.py:
bang_k_consolidate_scan and _clear on hand-built graphs of 130 nodes at R = 5, 16 and 64; bang_k_consolidate_gather for the three element types on
crafted rows (an empty list, exactly 512 and 513 candidates, p inside a removed row, duplicates, an excluded medoid as a live candidate), at every
vector layout and with graph entries 32 MiB apart; and the engine -- entries, codes, statistics and the remaining set on every delete set of
tests/consolidate_inputs.py, under the chunk hook, as a no-op, after its refusals, composed with inserts, and in three search forms afterwards.

Run time of the CPU references these tests wait for, measured on one core: see tests/test_consolidate_reference.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import consolidate_inputs as CI
import consolidate_reference as CR
import insert_inputs as I
import insert_reference as IR
from exact_reference import Reference

pytestmark = pytest.mark.gpu

K, L = 10, 48
MARK, SKIP = 0xCDCDCDCD, 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the three entries
# ---------------------------------------------------------------------------------------------------------------------
def _call(name, p):
    from bang_amd import binding as B
    fn = getattr(B.lib(), name)
    fn.argtypes = [C.c_void_p, C.c_void_p]
    B._check(fn(C.byref(p), None), name)
    B.sync()


def _table(p, graph_ptr, entry_len, dtype, D, R, n_nodes, medoid, bitmap_ptr):
    from bang_amd import binding as B
    p.d_graph, p.entry_len, p.dtype, p.D, p.R, p.n_nodes, p.medoid, p.d_excluded = graph_ptr, entry_len, B.DTYPE_CODE[dtype], D, R, n_nodes, medoid, bitmap_ptr


def _scan_gpu(graph_ptr, entry_len, dtype, D, R, n_nodes, medoid, excluded):
    """-> (affected ids ascending, the words behind the bitmap, abort word)"""
    from bang_amd import binding as B
    words = (n_nodes + 31) // 32
    bm = B.DeviceBuffer.from_numpy(CI.bitmap_of(excluded, n_nodes))
    aff = B.DeviceBuffer.from_numpy(np.concatenate([np.zeros(words, np.uint32), np.full(2, MARK, np.uint32)]))
    ab = B.DeviceBuffer(4)
    p = B.ConsolidateScanParams()
    _table(p, graph_ptr, entry_len, dtype, D, R, n_nodes, medoid, bm.ptr)
    p.d_affected, p.d_abort = aff.ptr, ab.ptr
    _call("bang_k_consolidate_scan", p)
    got, abort = aff.download(np.uint32, (words + 2,)), int(ab.download(np.uint32, (1,))[0])
    for b in (bm, aff, ab):
        b.free()
    ids = [i for i in range(words * 32) if (int(got[i >> 5]) >> (i & 31)) & 1]
    return ids, got[words:], abort


def _gather_gpu(graph_ptr, entry_len, dtype, D, R, n_nodes, medoid, excluded, nodes):
    """-> (cand ids [n][512], cand distance bits, offered, own, dropped, abort)"""
    from bang_amd import binding as B
    n = len(nodes)
    bm = B.DeviceBuffer.from_numpy(CI.bitmap_of(excluded, n_nodes))
    nd = B.DeviceBuffer.from_numpy(np.asarray(nodes, np.uint32))
    outs = [B.DeviceBuffer.from_numpy(np.full(k, MARK, np.uint32)) for k in (n * 512, n * 512, n, n)]
    ctl = B.DeviceBuffer(16)
    p = B.ConsolidateGatherParams()
    _table(p, graph_ptr, entry_len, dtype, D, R, n_nodes, medoid, bm.ptr)
    p.n_lists, p.d_nodes = n, nd.ptr
    p.d_cand_ids, p.d_cand_dists, p.d_offered, p.d_own_out = (b.ptr for b in outs)
    p.d_stats, p.d_abort = ctl.ptr, ctl.ptr + 4
    _call("bang_k_consolidate_gather", p)
    c = ctl.download(np.uint32, (2,))
    res = (outs[0].download(np.uint32, (n, 512)), outs[1].download(np.uint32, (n, 512)), outs[2].download(np.uint32, (n,)),
           outs[3].download(np.uint32, (n,)), int(c[0]), int(c[1]))
    for b in [bm, nd, ctl] + outs:
        b.free()
    return res


def _check_lists(ix, excluded, nodes, got, want_abort=0):
    """the gather's output for `nodes` against consolidate_reference.lists on ix"""
    ci, cd, offered, own, dropped, abort = got
    ref = Reference(ix)
    cl = CR.lists(ix, excluded)
    want_dropped = 0
    for i, p in enumerate(nodes):
        full = cl[int(p)].ids
        cand = full[:512]
        want_dropped += len(full) - len(cand)
        assert offered[i] == len(cand) and own[i] == p, (i, p, offered[i], len(cand))
        assert np.array_equal(ci[i, :len(cand)], cand), (p, "the list and its order")
        assert np.array_equal(cd[i, :len(cand)], _bits(ref.exact(cand, IR.vector_of(ref, int(p))))), (p, "the distance bits")
        assert (ci[i, len(cand):] == MARK).all() and (cd[i, len(cand):] == MARK).all(), (p, "written behind the list")
    assert dropped == want_dropped and abort == want_abort


@pytest.mark.parametrize("R", [5, 16, 64])
def test_scan_and_clear_on_the_hand_built_graph(R):
    """N = 130: degree 0 and degree R, a degree word above R, a removed id in the first and in the last slot and behind the degree, a removed node
    that lists removed nodes, the excluded medoid flagged as live, an id >= N that ends its row; then the clear: only rows of D change"""
    from bang_amd import binding as B
    graph, med, excluded, want, bad_node, bad_id = CI.scan_graph(R)
    el = graph.shape[1]
    g = B.DeviceBuffer.from_numpy(graph, slack=256)
    ids, behind, abort = _scan_gpu(g.ptr, el, "uint8", 16, R, CI.SCAN_N, med, excluded)
    assert ids == list(want) and (behind == MARK).all(), "the affected bitmap, and no word behind it"
    assert abort == 2, "the id >= N in node 127's row was not reported"
    assert np.array_equal(g.download(np.uint8, graph.shape), graph), "the scan wrote the graph"
    # without the bad id the abort word stays 0; without the medoid in the set the answer is the same
    sound = graph.copy()
    sound[bad_node, 16:].view(np.uint32)[2] = 9
    g.upload(sound)
    ids, _, abort = _scan_gpu(g.ptr, el, "uint8", 16, R, CI.SCAN_N, med, excluded[excluded != med])
    assert abort == 0 and ids == sorted(list(want) + [bad_node])          # (slot 2 of node 127, removed node 3, is now read)
    # the clear
    bm = B.DeviceBuffer.from_numpy(CI.bitmap_of(excluded, CI.SCAN_N))
    p = B.ConsolidateClearParams()
    _table(p, g.ptr, el, "uint8", 16, R, CI.SCAN_N, med, bm.ptr)
    _call("bang_k_consolidate_clear", p)
    after = g.download(np.uint8, graph.shape)
    expect = sound.copy()
    gone = [int(v) for v in excluded if v != med]
    expect[gone, 16:] = 0
    assert np.array_equal(after, expect), "the rows of D, and no other byte: vectors stay, the excluded medoid's row stays"
    assert after[med, 16:].any() and sound[gone, 16:].any()
    for b in (g, bm):
        b.free()


def _crafted(name):
    """-> (Index, excluded, nodes): I.get(name) with hand-made rows.  nv = 512 / R removed nodes with R live ids each;
      50: lists the nv of them -> exactly 512 candidates          51: a live id and the nv -> 513, one dropped
      52: lists 120 and 121, whose rows list removed nodes and 52 -> an empty list
      53: live, removed, the EXCLUDED MEDOID, removed; the removed rows list 53, each other, and ids twice
    and the first two nodes the index's own rows make affected."""
    ix, _ = I.get(name)
    R, med = ix.R, int(ix.medoid)
    nv = 512 // R
    vs = list(range(100, 100 + nv))
    assert med not in vs + [50, 51, 52, 53, 120, 121, 122, 123, 124, 1500, 1600, 1602, 1603]
    rows = {v: 200 + i * R + np.arange(R) for i, v in enumerate(vs)}
    rows.update({50: vs, 51: [1500] + vs, 52: [120, 121], 120: [121, 52, 122], 121: [122], 122: [],
                 53: [1600, 123, med, 124], 123: [53, 1602, 1603, 124, 1602], 124: [1603, 53, 1600]})
    ix = CI.with_rows(ix, rows)
    excluded = np.array(vs + [120, 121, 122, 123, 124, med], np.uint32)
    natural = [p for p in CR.lists(ix, excluded) if p not in (50, 51, 52, 53)][:2]
    return ix, excluded, [50, 51, 52, 53] + natural


@pytest.mark.parametrize("name", ["i8", "u8", "f32"])
def test_gather_on_crafted_rows(name):
    """six lists, the last workgroup half full; then a launch whose first node is an id outside the index"""
    from bang_amd import binding as B
    ix, excluded, nodes = _crafted(name)
    cl = CR.lists(ix, excluded)
    assert [len(cl[p].ids) for p in nodes[:4]] == [512, 513, 0, 7] and len(nodes) == 6
    assert list(cl[53].ids) == [1600, int(ix.medoid), 1602, 1603, 1602, 1603, 1600] and cl[53].lists_p
    g = B.DeviceBuffer.from_numpy(ix.graph, slack=256)
    args = (g.ptr, ix.entry_len, ix.dtype, ix.D, ix.R, ix.N, int(ix.medoid), excluded)
    got = _gather_gpu(*args, nodes)
    _check_lists(ix, excluded, nodes, got)
    assert got[4] == 1 and list(got[2][:4]) == [512, 512, 0, 7]
    ci, cd, offered, own, dropped, abort = _gather_gpu(*args, [ix.N + 3, 53])
    assert abort == 2 and offered[0] == 0 and own[0] == SKIP and (ci[0] == MARK).all()
    _check_lists(ix, excluded, [53], (ci[1:], cd[1:], offered[1:], own[1:], dropped, 0))
    assert np.array_equal(g.download(np.uint8, ix.graph.shape), ix.graph), "the gather wrote the graph"
    g.free()


@pytest.mark.parametrize("name", sorted(I.LAYOUTS))
def test_gather_every_layout(name):
    """the node's vector as the wave's query at the layouts the four indexes leave out; seven lists (a last workgroup of three waves)"""
    from bang_amd import binding as B
    ix, excluded, _ = CI.case("layout_" + name)
    nodes = [int(p) for p in CI.reference("layout_" + name)[1]["affected"][3:10]]
    g = B.DeviceBuffer.from_numpy(ix.graph, slack=256)
    got = _gather_gpu(g.ptr, ix.entry_len, ix.dtype, ix.D, ix.R, ix.N, int(ix.medoid), excluded, nodes)
    g.free()
    _check_lists(ix, excluded, nodes, got)
    assert (got[2] > ix.R).all()


def test_row_addressing_beyond_4_gib():
    """the graph entries 32 MiB apart: id * entry_len passes 4 GiB at id 128.  200 entries with random rows among them; the scan over all of them,
    the gather on affected nodes >= 128 whose removed neighbours and candidates lie there too, and the clear -- seen through a second gather,
    which then finds the removed rows empty"""
    import stretch_inputs as S
    from bang_amd import binding as B
    ix0, _ = S.get("i8_64_m16")
    NN, R = 200, ix0.R
    rng = np.random.default_rng(23)
    rows = {}
    for p in range(NN):
        ids = rng.choice(NN - 1, 12, replace=False)
        rows[p] = (ids + (ids >= p)).astype(np.uint32)
    ix = CI.with_rows(dataclasses.replace(ix0, N=NN, graph=ix0.graph[:NN].copy(), codes=ix0.codes[:NN], medoid=0), rows)
    excluded = np.array([5, 130, 150, 199], np.uint32)
    stride = S.stride_of(ix.entry_len)
    assert (NN - 1) * stride > (4 << 30) and stride % 4 == 0
    buf, ptr = S.stretched(ix.graph, stride)
    cl = CR.lists(ix, excluded)
    ids, _, abort = _scan_gpu(ptr, stride, ix.dtype, ix.D, R, NN, 0, excluded)
    assert abort == 0 and ids == sorted(cl) and max(ids) >= 128
    nodes = [p for p in sorted(cl) if p >= 128][:5] + [p for p in sorted(cl) if p < 128][:2]
    far = [p for p in nodes[:5] if any(v >= 128 for v in rows[p] if v in excluded)]
    assert far, "no far node lists a far removed node: the removed row's address would not pass 4 GiB"
    got = _gather_gpu(ptr, stride, ix.dtype, ix.D, R, NN, 0, excluded, nodes)
    _check_lists(ix, excluded, nodes, got)
    bm = B.DeviceBuffer.from_numpy(CI.bitmap_of(excluded, NN))
    p = B.ConsolidateClearParams()
    _table(p, ptr, stride, ix.dtype, ix.D, R, NN, 0, bm.ptr)
    _call("bang_k_consolidate_clear", p)
    bm.free()
    cleared = CI.with_rows(ix, {int(v): [] for v in excluded})
    got = _gather_gpu(ptr, stride, ix.dtype, ix.D, R, NN, 0, excluded, nodes)
    buf.free()
    _check_lists(cleared, excluded, nodes, got)
    assert (got[2] < 12).all()


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def _engine(ix, capacity, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, **(dict(capacity=capacity) if capacity is not None else {}), **opts)
    e.load_index(ix)
    return e


def _want_stats(st):
    return dict(rows=st["rows"], removed=st["removed"], dropped=st["dropped"], still_excluded=st["still_excluded"])


@pytest.mark.parametrize("name", sorted(CI.CASES))
def test_consolidate_matches_the_reference_byte_for_byte(name):
    ix, x, alpha = CI.case(name)
    ix2, st, remaining = CI.reference(name)
    with _engine(ix, ix.N) as e:                                           # (capacity = N is enough)
        e.set_excluded(x)
        got = e.consolidate(alpha)
        assert got == _want_stats(st)
        assert np.array_equal(e.entries(0, ix.N), ix2.graph)
        assert np.array_equal(e.codes(0, ix.N), ix.codes)
        assert e.num_nodes() == ix.N and e.stats()["excluded"] == len(remaining)
        assert e.consolidate_stats() == dict(consolidated_rows=st["rows"], removed=st["removed"], consolidate_dropped=st["dropped"])
        t = e.consolidate_times()
        assert t["total"] > 0 and t["total"] >= t["rows"] > 0
        # a second call has nothing new to fold: nothing changes, byte for byte, and the totals stay
        assert e.consolidate(alpha) == dict(rows=0, removed=0, dropped=0, still_excluded=len(remaining))
        assert np.array_equal(e.entries(0, ix.N), ix2.graph)
        assert e.consolidate_stats()["consolidated_rows"] == st["rows"] and e.stats()["excluded"] == len(remaining)


def test_an_empty_set_is_a_no_op():
    ix, _, _ = CI.case("i8_ball24")
    with _engine(ix, ix.N + 5) as e:
        assert e.consolidate() == dict(rows=0, removed=0, dropped=0, still_excluded=0)
        assert np.array_equal(e.entries(0, ix.N), ix.graph) and np.array_equal(e.codes(0, ix.N), ix.codes)
        assert e.consolidate_stats() == dict(consolidated_rows=0, removed=0, consolidate_dropped=0)


@pytest.mark.parametrize("chunk", ["1", "7", "0", "100000"])
def test_the_chunk_hook_changes_nothing(chunk, monkeypatch):
    """1 and 7 affected nodes per gather / sort / prune launch give the bytes of the unchunked call (the reference knows no chunks); 0 is taken as
    1 and 100000 as 8192 (the clamp)"""
    name = "cut_ball12" if chunk == "7" else "i8_ball8_med"
    ix, x, alpha = CI.case(name)
    ix2, st, _ = CI.reference(name)
    monkeypatch.setenv("BANG_CONSOLIDATE_CHUNK", chunk)
    with _engine(ix, ix.N) as e:
        e.set_excluded(x)
        assert e.consolidate(alpha) == _want_stats(st)
        assert np.array_equal(e.entries(0, ix.N), ix2.graph)


def test_refusals_leave_no_trace():
    import bang_amd
    import stretch_inputs as S
    from bang_amd import BangError
    ix, x, alpha = CI.case("i8_ball8_med")
    ix2, st, _ = CI.reference("i8_ball8_med")
    with _engine(ix, None) as e:                                           # no capacity
        e.set_excluded(x)
        with pytest.raises(BangError, match="bang_consolidate.*capacity"):
            e.consolidate(alpha)
        assert e.stats()["excluded"] == len(x)
    wide, _ = S.get("u8_48")                                               # 8-bit, D / 16 = 3: outside bang_search_can_rerank
    with _engine(wide, wide.N) as e:
        e.set_excluded([1, 2])
        with pytest.raises(BangError, match="bang_consolidate.*layout"):
            e.consolidate(alpha)
        assert np.array_equal(e.entries(0, wide.N), wide.graph) and e.stats()["excluded"] == 2
    with _engine(ix, ix.N) as e:
        e.set_excluded(x)

        def refused(match, a=alpha):
            with pytest.raises(BangError, match="bang_consolidate.*" + match):
                e.consolidate(a)
        for a in (float("nan"), float("inf"), 0.99, 8.5):
            refused("alpha", a)
        e.set_searchparams(K, 40)
        e.alloc(8)
        refused("allocation")
        e.free()
        e.set_searchparams(K, 40, bang_amd.DIST_MIPS)
        refused("MIPS")
        e.set_searchparams(K, 40)
        assert np.array_equal(e.entries(0, ix.N), ix.graph) and e.stats()["excluded"] == len(x), "a refused call left a trace"
        assert e.consolidate_stats() == dict(consolidated_rows=0, removed=0, consolidate_dropped=0)
        e.set_labels(np.ones(ix.N, np.uint32))                             # a label table may stay set: N does not change
        assert e.consolidate(alpha) == _want_stats(st)                     # ... and the engine still consolidates
        assert np.array_equal(e.entries(0, ix.N), ix2.graph)


def test_composition_with_inserts():
    """insert, exclude 8 inserted and 16 old ids, consolidate, insert again: the engine equals the references applied in that order"""
    ix, v, Lb, alpha = I.case("i8_a12")
    ix1, _ = I.reference("i8_a12")
    near = CI.ball(ix1, ix.N + 10, 60)                                     # around an inserted node that stays: its row is affected
    x = np.concatenate([ix.N + np.arange(8), near[near < ix.N][:16]]).astype(np.uint32)
    ix2, st, remaining = CR.consolidate(ix1, x, 1.2)
    assert len(remaining) == 0 and st["removed"] == 24 and (st["affected"] >= ix.N).any(), "no inserted row is affected"
    v2 = I.batch(ix2, 16, 9)
    ix3, _ = IR.insert(ix2, v2, Lb, alpha)
    with _engine(ix, ix.N + len(v) + len(v2)) as e:
        assert e.insert(v, Lb, alpha) == ix.N
        e.set_excluded(x)
        assert e.consolidate(1.2) == _want_stats(st)
        assert np.array_equal(e.entries(0, ix2.N), ix2.graph) and np.array_equal(e.codes(0, ix2.N), ix2.codes)
        assert e.insert(v2, Lb, alpha) == ix2.N
        assert np.array_equal(e.entries(0, ix3.N), ix3.graph) and np.array_equal(e.codes(0, ix3.N), ix3.codes)
        assert not np.isin(ix3.adjacency()[np.arange(ix3.R)[None, :] < ix3.degrees()[:, None]], x).any(), "a new row lists a removed node"


# form -> the options of bang_alloc
FORMS = {"exact": dict(distance=1, search=1), "pq": dict(distance=0, search=1), "loop": dict(distance=0, search=0)}


def _search(e, q, form):
    for key, val in FORMS[form].items():
        e.set_option(key, val)
    e.set_searchparams(K, L)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    st = e.stats()
    out = (ids, _bits(d), e.query_counters(q.shape[0]))
    e.free()
    return out, st


def _form_reference(ix2, q, form):
    if form == "exact":
        ids, d, st = Reference(ix2).search(q, K, L, "exact")
        return ids, _bits(d), st
    from oracle import oracle as O
    ids, d, st = O.Oracle(ix2).search(q, K, L, with_stats=True)
    return ids, _bits(d), (st if form == "pq" else None)                  # (the per-iteration kernels keep no per-query counters)


@pytest.mark.parametrize("name", ["i8_ball24", "i8_ball8_med"])
def test_searches_after_consolidation(name):
    """24 queries -- 16 of the index's and the vectors of 8 removed nodes --, k = 10, L = 48, on the exact walk, the query-resident PQ kernel and
    the launch-per-iteration loop: before the deletes they return removed ids; afterwards none, the answers are the CPU reference's on Index' (where
    the set ends empty) and those of a fresh engine loaded from the export with the remaining set applied"""
    ix, x, alpha = CI.case(name)
    ix2, st, remaining = CI.reference(name)
    gone = x[x != ix.medoid]
    q = np.ascontiguousarray(np.concatenate([I.get("i8")[1][:16], ix.vectors()[gone[:8]]]))
    with _engine(ix, ix.N) as e:
        for form in FORMS:
            (ids, _, _), _ = _search(e, q, form)
            assert np.isin(ids, gone).sum() >= 8, (form, "the queries do not find the nodes to be removed: the test would show nothing")
        e.set_excluded(x)
        assert e.consolidate(alpha) == _want_stats(st)
        exported = e.export_index(ix)
        assert np.array_equal(exported.graph, ix2.graph)
        mine = {}
        for form in FORMS:
            mine[form], stats = _search(e, q, form)
            assert not np.isin(mine[form][0], gone).any(), (form, "a removed id was returned")
            assert stats["excluded"] == len(remaining)
            if form == "pq" and len(remaining) == 0:
                assert stats["rerank_fused"] == 1, "the set is empty again: the re-rank runs fused"
            if len(remaining) == 0:
                for got, want, part in zip(mine[form], _form_reference(ix2, q, form), ("ids", "distance bits", "counters")):
                    assert want is None or np.array_equal(got, want), (form, part, "reference")
            else:
                assert not (mine[form][0] == ix.medoid).any(), (form, "the excluded medoid was returned")
    with _engine(exported, None) as f:
        if len(remaining):
            f.set_excluded(remaining)
        for form in FORMS:
            theirs, _ = _search(f, q, form)
            for got, want, part in zip(theirs, mine[form], ("ids", "distance bits", "counters")):
                assert np.array_equal(got, want), (form, part, "fresh engine")
