"""Excluded ids (lazy deletes: Engine.set_excluded, bang_k_cand_live / bang_k_worklist_pick of csrc/bang_exclude.hip) on a GPU, against the
composition of tests/exclude_reference.py: ids and distance bits of the masked answer, and -- the walk is untouched -- the four per-query
counters and the candidate log of the same engine run with the set empty, which are the reference's.  32 queries per fixture; worklists of 10,
37 and 152 (k = 10, and k = L at L = 37); the PQ walks in every form whose re-rank finds a vector by its id, the exact-distance walks on both
placements, with a beam, on a wide layout and on an fp16 table; the chain input for candidate logs of exactly 60, 87 and 202 entries (one, two
and four 64-entry pieces).  Then: the set cleared restores today's run; one allocation queried twice; two lanes; one wave; results into device
buffers; the refusals; the CLI under BANG_EXCLUDE_FILE."""
import os
import subprocess

import numpy as np
import pytest

import base_forms as F
import beam_inputs as BI
import edge_inputs as E
import exclude_reference as X

pytestmark = pytest.mark.gpu

K = 10
NQ = 32
LS = (10, 37, 152)
PAD = int(X.PAD_ID)
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(e, q, k, L, mask, extra=50, distfn=0, Qcap=None):
    """A loaded, unallocated engine: set the mask (None: never touched; empty: set, then cleared), run one batch, free.
    -> (ids, dists, counters, log, counts, stats)"""
    Q = q.shape[0]
    if mask is not None:
        if len(mask) == 0:
            e.set_excluded([0, 1])
            e.clear_excluded()
        else:
            e.set_excluded(mask)
    e.set_searchparams(k, L, distfn)
    e.alloc(Q if Qcap is None else Qcap)
    e.init(Q)
    ids, d = e.query(q)
    out = (ids, d, e.query_counters(Q)) + e.candidate_log(Q, L, extra) + (e.stats(),)
    e.free()
    return out


def _same_results(got, want_ids, want_d, what=""):
    assert np.array_equal(got[0], want_ids), what
    assert np.array_equal(_bits(got[1]), _bits(want_d)), what


def _same_walk(got, base, what="", iterations=True):
    """Counters and candidate log of two runs are the same."""
    c0 = 0 if iterations else 1
    assert np.array_equal(got[2][:, c0:], base[2][:, c0:]), what
    assert np.array_equal(got[4], base[4]), what
    for i in range(len(got[4])):
        assert np.array_equal(got[3][i, :got[4][i]], base[3][i, :base[4][i]]), (what, i)


def _ref_walk(got, st, log, cnt, what="", iterations=True):
    c0 = 0 if iterations else 1
    assert np.array_equal(got[2][:, c0:], st[:, c0:]), what
    if log is not None:
        assert np.array_equal(got[4], cnt), what
        for i in range(len(cnt)):
            assert np.array_equal(got[3][i, :cnt[i]], log[i, :cnt[i]]), (what, i)


# ---------------------------------------------------------------------------------------------------------------------
# the PQ walks
# ---------------------------------------------------------------------------------------------------------------------
PQ_FORMS = {                                                  # form -> (engine options, reference walk, log entries beyond L)
    "self":      (dict(graph=1, search=1), "split", 50),      # (would have been fused)
    "self_pull": (dict(graph=0, pull=1), "split", 50),        # rows pulled from host memory, vectors in the HBM table
    "lut":       (dict(graph=1, pq=1, search=1), "split", 50),
    "inmemory":  (dict(graph=1, semantics=1), "inmemory", 120),
    "word":      (dict(graph=1, filter_layout=1), "word", 50),
}


def _pq_ref(name, ix, q, L, walk, mips=False):
    def make():
        if walk == "inmemory":
            return X.walk_inmemory(ix, q, K, L)
        return X.walk_base(ix, q, K, L, layout=walk, mips=mips)
    return _cached((name, q.shape, L, walk, mips), make)


def _fused_expected(form, ix, mips=False):
    if mips:
        return 0                                              # (the fused re-rank takes no MIPS padding)
    if form == "self" or form == "inmemory" or form == "word":
        return int(F.fusable(ix.dtype, ix.D, ix.entry_len))
    if form == "self_pull":
        return int(F.fusable(ix.dtype, ix.D, ix.D * F.tsize(ix.dtype)))
    return 0


def _pq_case(name, ix, q, form, Ls, masks, monkeypatch=None, distfn=0, mips=False, k_equals_L=True):
    import bang_amd
    opts, walk, extra = PQ_FORMS[form]
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        for L in Ls:
            if L != Ls[0]:
                e.clear_excluded()                                         # (the first L runs on an engine whose set was never touched)
            ids_r, d_r, st_r, log_r, cnt_r = _pq_ref(name, ix, q, L, walk, mips)
            base = _run(e, q, K, L, None, extra, distfn)
            _same_results(base, ids_r, d_r, (form, L, "unmasked"))
            _ref_walk(base, st_r, log_r, cnt_r, (form, L, "unmasked"))
            s = base[5]
            assert s["rerank_fused"] == _fused_expected(form, ix, mips) and s["exclude_launches"] == 0 and s["excluded"] == 0, s
            none = _run(e, q, K, L, [], extra, distfn)                     # `none`: set, then cleared -- today's run
            _same_results(none, ids_r, d_r, (form, L, "none"))
            _same_walk(none, base, (form, L, "none"))
            s = none[5]
            assert s["rerank_fused"] == _fused_expected(form, ix, mips) and s["exclude_launches"] == 0 and s["excluded"] == 0, s
            for mname, mask in masks(ix, ids_r[:, 0]):
                ks = (K, L) if (k_equals_L and L == 37 and mname in ("rand30", "all_but_one", "positions")) else (K,)
                for k in ks:
                    got = _run(e, q, k, L, mask, extra, distfn)
                    want = X.rerank_all(ix, q, log_r, cnt_r, mask, k, mips)
                    _same_results(got, want[0], want[1], (form, L, mname, k))
                    _same_walk(got, base, (form, L, mname, k))
                    _ref_walk(got, st_r, log_r, cnt_r, (form, L, mname, k))
                    s = got[5]
                    assert s["rerank_fused"] == 0 and s["exclude_launches"] == 1 and s["excluded"] == len(np.unique(mask)), s
        e.unload()


def _named_masks(ix, rank0):
    return [(m, X.make_mask(m, ix, rank0)) for m in X.MASKS]


@pytest.mark.parametrize("form", list(PQ_FORMS))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_pq_walks(request, fixture, form):
    ix, q, _, _ = request.getfixturevalue(fixture)
    _pq_case(fixture, ix, np.ascontiguousarray(q[:NQ]), form, LS, _named_masks)


def test_pq_walk_mips(small_f32):
    import bang_amd
    ix, q, _, _ = small_f32
    q1 = np.ascontiguousarray(q[:NQ, :-1])
    _pq_case("small_f32", ix, q1, "self", (37,), _named_masks, distfn=bang_amd.DIST_MIPS, mips=True)


def _chain_masks(ix, rank0):
    n = int(rank0[0]) + 1                                     # the log is 0 .. n - 1 and its last node is the nearest
    return [("nearest", np.array([n - 1], np.uint32)),
            ("positions", np.array([x for x in (0, 63, 64, n - 1) if x < n], np.uint32)),
            ("five_left", np.arange(5, 256, dtype=np.uint32)),
            ("duplicates", np.array([3, 3, n - 2, 3, n - 2], np.uint32)),
            ("all_but_one", X.make_mask("all_but_one", ix)),
            ("all", np.arange(ix.N, dtype=np.uint32))]


@pytest.mark.parametrize("form", ("self", "self_pull", "inmemory"))
def test_chain_logs_of_one_two_and_four_pieces(form):
    """The chain runs to the iteration cap: logs of exactly 60, 87 and 202 entries (semantics = 1: longer, up to the chain's 256 nodes).  `all`: nothing is left."""
    ix, q = E.chain()
    _pq_case("chain", ix, q, form, LS, _chain_masks)


# ---------------------------------------------------------------------------------------------------------------------
# the exact-distance walks
# ---------------------------------------------------------------------------------------------------------------------
EXACT_FORMS = {
    "hbm":        (dict(graph=1, distance=1), 1),
    "pull":       (dict(graph=0, pull=1, distance=1), 1),
    "hbm_beam2":  (dict(graph=1, distance=1, beam=2), 2),
    "pull_beam2": (dict(graph=0, pull=1, distance=1, beam=2), 2),
}


def _exact_case(name, ix, q, opts, beam, Ls, masks, ref_ix=None):
    import bang_amd
    rix = ix if ref_ix is None else ref_ix
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        for L in Ls:
            if L != Ls[0]:
                e.clear_excluded()
            wl_i, wl_d, st_r = _cached((name, q.shape, L, "exact", beam), lambda: X.walk_exact(rix, q, L, beam))
            base = _run(e, q, K, L, None)
            _same_results(base, np.ascontiguousarray(wl_i[:, :K]), np.ascontiguousarray(wl_d[:K]), (name, L, "unmasked"))
            _ref_walk(base, st_r, None, None, (name, L, "unmasked"))
            assert base[5]["exclude_launches"] == 0 and base[5]["excluded"] == 0 and base[5]["front_launches"] == 1, base[5]
            none = _run(e, q, K, L, [])
            _same_results(none, base[0], base[1], (name, L, "none"))
            _same_walk(none, base, (name, L, "none"))
            assert none[5]["exclude_launches"] == 0 and none[5]["excluded"] == 0, none[5]
            for mname, mask in masks(ix, wl_i[:, 0]):
                for k in ((K, L) if L == 37 and mname in ("rand30", "all_but_one") else (K,)):
                    got = _run(e, q, k, L, mask)
                    want = X.worklist_all(wl_i, wl_d, mask, k)
                    _same_results(got, want[0], want[1], (name, L, mname, k))
                    _same_walk(got, base, (name, L, mname, k))
                    _ref_walk(got, st_r, None, None, (name, L, mname, k))
                    s = got[5]
                    assert s["exclude_launches"] == 1 and s["excluded"] == len(np.unique(mask)) and s["front_launches"] == 1, s
        e.unload()


@pytest.mark.parametrize("form", list(EXACT_FORMS))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_exact_walks(request, fixture, form):
    ix, q, _, _ = request.getfixturevalue(fixture)
    opts, beam = EXACT_FORMS[form]
    _exact_case(fixture, ix, np.ascontiguousarray(q[:NQ]), opts, beam, LS, _named_masks)


def test_exact_walk_on_a_wide_layout():
    import highdim_inputs as H
    ix, q = H.get("u8_48")
    _exact_case("u8_48", ix, q, dict(graph=1, distance=1), 1, (37,), _named_masks)


def test_exact_walk_on_an_fp16_table(small_f32):
    """graph = host, pulled rows, vectors_fp16 = 1: the walk of the index with its vectors rounded to fp16."""
    import fp16_inputs as H16
    ix, q, _, _ = small_f32
    _exact_case("small_f32_r", ix, np.ascontiguousarray(q[:NQ]), dict(graph=0, pull=1, distance=1, vectors_fp16=1), 1, (37,), _named_masks,
                ref_ix=H16.rounded(ix))


def test_pq_walk_on_an_fp16_table(small_f32):
    """... and the re-rank launch that reads that table (bang_k_rerank_f16) takes the live list as well."""
    import bang_amd
    import fp16_inputs as H16
    ix, q, _, _ = small_f32
    q = np.ascontiguousarray(q[:NQ])
    rix = H16.rounded(ix)
    ids_r, d_r, st_r, log_r, cnt_r = _pq_ref("small_f32_r", rix, q, 37, "split")
    mask = X.make_mask("rand30", ix)
    with bang_amd.Engine(ix.dtype, graph=0, pull=1, vectors_fp16=1) as e:
        e.load_index(ix)
        got = _run(e, q, K, 37, mask)
        want = X.rerank_all(rix, q, log_r, cnt_r, mask, K)
        _same_results(got, want[0], want[1])
        _ref_walk(got, st_r, log_r, cnt_r)
        assert got[5]["vectors_fp16"] == 1 and got[5]["exclude_launches"] == 1, got[5]
        e.unload()


def _toy_masks(sets):
    return lambda ix, r0: [(str(s), np.array(s, np.uint32)) for s in sets]


@pytest.mark.parametrize("form", list(EXACT_FORMS))
def test_exact_walks_on_the_toy_inputs(form):
    """shared_child without its nearest node; row_dup without node 2 (both copies go) and without node 4 (both copies of 2 stay); the chain,
    whose worklist is full, at k = 10 of L = 10."""
    opts, beam = EXACT_FORMS[form]
    ix, q = BI.shared_child()
    _exact_case("shared_child", ix, q, opts, beam, (10,), _toy_masks(([3], [3, 1, 0], [0, 1, 2, 3, 4, 5])))
    ix, q = BI.row_dup()
    _exact_case("row_dup", ix, q, opts, beam, (10,), _toy_masks(([2], [4], [4, 5])))
    ix, q = E.chain()
    _exact_case("chain", ix, q, opts, beam, (10, 152), _chain_masks)


# ---------------------------------------------------------------------------------------------------------------------
# one allocation twice; lanes; one wave; device buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", (dict(graph=1, search=1), dict(graph=1, distance=1)), ids=("pq", "exact"))
def test_init_and_query_twice_on_one_allocation(small_u8, opts):
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    mask = X.make_mask("rand30", ix)
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        e.set_excluded(mask)
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        runs = []
        for nb in (NQ, NQ, 7):
            e.init(nb)
            ids, d = e.query(q[:nb])
            runs.append((ids, d, e.query_counters(nb)))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])) and np.array_equal(runs[0][2], runs[1][2])
        assert np.array_equal(runs[2][0], runs[0][0][:7]) and np.array_equal(_bits(runs[2][1]), _bits(runs[0][1][:, :7]))
        if "distance" in opts:
            wl = _cached(("small_u8", q.shape, 37, "exact", 1), lambda: X.walk_exact(ix, q, 37, 1))
            want = X.worklist_all(wl[0], wl[1], mask, K)
        else:
            r = _pq_ref("small_u8", ix, q, 37, "split")
            want = X.rerank_all(ix, q, r[3], r[4], mask, K)
        _same_results(runs[0], want[0], want[1])
        e.free()
        e.unload()


@pytest.mark.parametrize("opts", (dict(graph=1, search=0, lanes=2), dict(graph=0, pull=0, search=0, vectors=1, lanes=2)), ids=("hbm", "walker"))
def test_two_lanes(small_f32, opts):
    """The launch-per-iteration loop on two lanes: each lane compacts and re-ranks its own queries."""
    import bang_amd
    ix, q, _, _ = small_f32
    q = np.ascontiguousarray(q[:17])
    mask = X.make_mask("rand30", ix)
    r = _pq_ref("small_f32", ix, q, 37, "split")
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        base = _run(e, q, K, 37, None, Qcap=NQ)
        _same_results(base, r[0], r[1])
        got = _run(e, q, K, 37, mask, Qcap=NQ)
        want = X.rerank_all(ix, q, r[3], r[4], mask, K)
        _same_results(got, want[0], want[1])
        _same_walk(got, base, iterations=False)
        _ref_walk(got, r[2], r[3], r[4], iterations=False)
        assert got[5]["lanes"] == 2 and got[5]["exclude_launches"] == 2 and base[5]["exclude_launches"] == 0, got[5]
        e.unload()


@pytest.mark.parametrize("form", ("self", "self_pull"))
def test_one_wave_per_workgroup(small_u8, form, monkeypatch):
    ix, q, _, _ = small_u8
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    _pq_case("small_u8", ix, np.ascontiguousarray(q[:NQ]), form, (37,), lambda ix_, r0: [("rand30", X.make_mask("rand30", ix_))], k_equals_L=False)


def test_one_wave_per_workgroup_exact(small_u8, monkeypatch):
    ix, q, _, _ = small_u8
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    _exact_case("small_u8", ix, np.ascontiguousarray(q[:NQ]), dict(graph=1, distance=1), 1, (37,), lambda ix_, r0: [("top", X.make_mask("top", ix_, r0))])


@pytest.mark.parametrize("opts", (dict(graph=1, search=1), dict(graph=1, distance=1), dict(graph=0, pull=1, distance=1, beam=2)),
                         ids=("pq", "exact", "exact_pull_beam2"))
@pytest.mark.parametrize("with_dists", (True, False))
def test_results_into_device_buffers(small_u8, opts, with_dists):
    import torch
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    mask = X.make_mask("top", ix, _pq_ref("small_u8", ix, q, 37, "split")[0][:, 0])
    if "distance" in opts:
        beam = opts.get("beam", 1)
        wl = _cached(("small_u8", q.shape, 37, "exact", beam), lambda: X.walk_exact(ix, q, 37, beam))
        want = X.worklist_all(wl[0], wl[1], mask, K)
    else:
        r = _pq_ref("small_u8", ix, q, 37, "split")
        want = X.rerank_all(ix, q, r[3], r[4], mask, K)
    d_ids = torch.zeros((NQ, K), dtype=torch.int64, device="cuda")
    d_d = torch.zeros((K, NQ), dtype=torch.float32, device="cuda")
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        e.set_excluded(mask)
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        e.init(NQ)
        e.query_dev(q, d_ids.data_ptr(), d_d.data_ptr() if with_dists else 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), want[0])
        if with_dists:
            assert np.array_equal(d_d.cpu().numpy().view(np.uint32), _bits(want[1]))
        else:
            assert not d_d.cpu().numpy().any()
        assert e.stats()["exclude_launches"] == 1
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# call order and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_call_order_and_out_of_range(small_u8):
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    r = _pq_ref("small_u8", ix, q, 37, "split")
    mask = X.make_mask("edges", ix)
    with bang_amd.Engine(ix.dtype, graph=1) as e:
        with pytest.raises(bang_amd.BangError, match="no index is loaded"):
            e.set_excluded(mask)
        e.load_index(ix)
        e.set_excluded(mask)
        with pytest.raises(bang_amd.BangError, match="out of range"):      # an id equal to N: refused, and the set stays what it was
            e.set_excluded([1, 2, ix.N])
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        for call in (lambda: e.set_excluded([5]), e.clear_excluded):
            with pytest.raises(bang_amd.BangError, match="bang_alloc"):    # the rule of the options consumed by bang_alloc
                call()
        e.init(NQ)
        ids, d = e.query(q)
        want = X.rerank_all(ix, q, r[3], r[4], mask, K)
        _same_results((ids, d), want[0], want[1])
        assert e.stats()["excluded"] == len(mask)
        e.free()
        e.set_excluded([ix.N - 1])                                         # the last id is fine, and REPLACES the set
        got = _run(e, q, K, 37, None)
        want = X.rerank_all(ix, q, r[3], r[4], [ix.N - 1], K)
        _same_results(got, want[0], want[1])
        assert got[5]["excluded"] == 1
        e.unload()                                                         # drops the set
        e.load_index(ix)
        got = _run(e, q, K, 37, None)
        _same_results(got, r[0], r[1])
        assert got[5]["excluded"] == 0 and got[5]["exclude_launches"] == 0
        e.unload()


@pytest.mark.parametrize("opts", (dict(graph=0, vectors=0), dict(graph=0, vectors=0, search=0), dict(graph=0, vectors=0, persistent=0)),
                         ids=("host_paced", "search_0", "persistent_0"))
def test_vector_log_forms_are_refused(small_i8, opts):
    """vectors = 0: the re-rank reads a vector log, whose rows compaction would break.  Refused at bang_alloc with `excluded` in the message;
    with the set cleared the same engine allocates and runs."""
    import bang_amd
    from oracle import oracle as O
    ix, q, _, _ = small_i8
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        e.set_excluded([1, 2, 3])
        e.set_searchparams(K, 24)
        with pytest.raises(bang_amd.BangError, match="excluded"):
            e.alloc(8)
        e.clear_excluded()
        got = _run(e, np.ascontiguousarray(q[:8]), K, 24, None)
        want = O.Oracle(ix).search(q[:8], K, 24)
        _same_results(got, want[0], want[1])
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the environment variable: bang.h callers and the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_exclude_file_is_read_by_every_load(small_i8, tmp_path, monkeypatch):
    import bang_amd
    from bang_amd import formats
    ix, q, _, _ = small_i8
    q = np.ascontiguousarray(q[:NQ])
    mask = X.make_mask("rand30", ix)
    path = str(tmp_path / "x.bin")
    formats.write_bin(path, mask.reshape(-1, 1))
    r = _pq_ref("small_i8", ix, q, 24, "split")
    want = X.rerank_all(ix, q, r[3], r[4], mask, K)
    monkeypatch.setenv("BANG_EXCLUDE_FILE", path)
    with bang_amd.Engine(ix.dtype, graph=1) as e:
        e.load_index(ix)                                                   # bang_load_mem_e
        got = _run(e, q, K, 24, None)
        _same_results(got, want[0], want[1])
        assert got[5]["excluded"] == len(mask)
        e.unload()
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    with bang_amd.Engine(ix.dtype, graph=0) as e:
        e.load(prefix)                                                     # bang_load_e (streamed: pulled rows)
        got = _run(e, q, K, 24, None)
        _same_results(got, want[0], want[1])
        e.unload()
    bad = str(tmp_path / "bad.bin")
    formats.write_bin(bad, np.array([[1], [ix.N]], np.uint32))
    odd = str(tmp_path / "odd.bin")
    with open(odd, "wb") as f:                                             # two columns, and a byte too many
        f.write(np.array([3, 2], np.int32).tobytes() + bytes(25))
    for p, word in ((bad, "out of range"), (str(tmp_path / "missing.bin"), "cannot be opened"), (odd, "not a .bin file")):
        monkeypatch.setenv("BANG_EXCLUDE_FILE", p)
        with bang_amd.Engine(ix.dtype, graph=1) as e:
            with pytest.raises(bang_amd.BangError) as err:
                e.load_index(ix)
            assert word in str(err.value) and p in str(err.value), str(err.value)
            monkeypatch.delenv("BANG_EXCLUDE_FILE")
            e.load_index(ix)                                               # (the failed load left nothing behind)
            e.unload()


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_EXCLUDE_FILE=... BANG_GRAPH=device bang_search (interactive L) prints its usual table; its recall at each L is that of the helper's ids."""
    import bang_amd
    from bang_amd import formats
    from oracle import oracle as O
    ix, q, gt_i, gt_d = small_i8
    mask = X.make_mask("rand30", ix)
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    formats.write_bin(str(tmp_path / "q.bin"), q)
    formats.write_truthset(str(tmp_path / "gt.bin"), gt_i, gt_d)
    formats.write_bin(str(tmp_path / "x.bin"), mask.reshape(-1, 1))
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    Ls = (10, 37)
    env = dict(os.environ, BANG_EXCLUDE_FILE=str(tmp_path / "x.bin"), BANG_GRAPH="device")
    out = subprocess.run([exe, prefix, str(tmp_path / "q.bin"), str(tmp_path / "gt.bin"), str(q.shape[0]), "10", "int8", "l2"],
                         input="".join(f"{L}\ny\n" for L in Ls[:-1]) + f"{Ls[-1]}\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split("\t") for l in out.stdout.splitlines() if l[:1].isdigit() and l.count("\t") == 3]
    assert "10-r@10" in out.stdout and sorted({int(r[0]) for r in rows}) == list(Ls)
    for L in Ls:
        r = _pq_ref("small_i8_all", ix, q, L, "split")
        ids, _ = X.rerank_all(ix, q, r[3], r[4], mask, K)
        unmasked = f"{float(np.float32(O.recall(gt_i, gt_d, r[0], 10))):.2f}"
        want = f"{float(np.float32(O.recall(gt_i, gt_d, ids, 10))):.2f}"
        got = [r_[3].strip() for r_ in rows if int(r_[0]) == L]
        assert want != unmasked                                            # (a run that ignored the file would print this)
        assert len(got) == 5 and all(g == want for g in got), (L, got, want)
