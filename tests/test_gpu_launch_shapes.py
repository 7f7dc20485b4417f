"""Every wave-resident search kernel in FULL workgroups (tests/launch_shapes.py: one workgroup of every wave that fits with two queries per wave;
three workgroups of five waves with 17 queries from the hand-out counter; the whole chip in full workgroups), against the CPU references of the
families' own files, bit for bit: ids, distance bits, the four per-query counters, the candidate log where the family's reference has one, `matched`
for the label filters, and counts, offered, lims, hit ids and hit distance bits for range search.  The other GPU files launch their 12 to 64 queries
as that many workgroups of ONE wave: a slice of LDS that overlaps its neighbour's, or per-query state that survives the hand-out, changes no answer
there.

Every case first asserts the (workgroups, waves) of its launch, from the geometry export of the family with the dtype, L, batch and caps the engine
uses -- none passes on a one-wave-per-workgroup launch -- then runs one engine on one batch (the range cases: one batch per radius set and
capacity).  The references walk the base queries only, once per (input, L); a batch larger than the input repeats its queries, and a copy must
return the bits of the original."""
import numpy as np
import pytest

import base_forms as F
import exclude_reference as X
import instance_inputs as I
import labels_inputs as LI
import labels_reference as LR
import launch_shapes as S
import range_inputs as RI
import range_reference as RR
import wordfilter_inputs as WI

pytestmark = pytest.mark.gpu

NQ = S.NQ


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(monkeypatch, family, shape, L, Q, min_waves=S.MIN_WAVES, **kw):
    """Sets the caps of `shape` and asserts that the launch the engine is about to make reaches it.  Q: the queries of ONE launch."""
    S.set_caps(monkeypatch, shape)
    full = S.geometry(family, L, S.FULL_Q, "full_chip", **kw)
    S.assert_reached(shape, S.geometry(family, L, Q, shape, **kw), Q, full, min_waves, S.rounds_of(family))
    default = S.geometry(family, L, NQ, "full_chip", **kw)                  # what the other files run: NQ workgroups of one wave
    assert default == (NQ, 1), default


def _engine(ix, options, **more):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, **dict(options, **more))
    try:
        e.load_index(ix)
    except BaseException:
        e.close()
        raise
    return e


def _run(e, q, k, L, filters=None, radii=None, cap=None):
    """One batch on a loaded engine -> dict; the allocation is freed"""
    Q = q.shape[0]
    if cap is not None:
        e.set_option("range_hits", cap)
    e.set_searchparams(k, L)
    e.alloc(Q)
    if filters is not None:
        e.set_filters(*filters)
    if radii is not None:
        e.set_radii(radii)
    e.init(Q)
    ids, d = e.query(q)
    log, log_n = e.candidate_log(Q, L)
    out = dict(ids=ids, d=d, counters=e.query_counters(Q), log=log, log_n=log_n, stats=e.stats())
    if filters is not None:
        out["matched"] = e.matched_counts(Q)
    if radii is not None:
        out["counts"], out["offered"] = e.range_counts(Q)
        out["lims"], out["hit_ids"], out["hit_d"] = e.range_results(Q)
    e.free()
    return out


def _check_walk(got, want, what):
    """want = (ids [Q][k], dists [k][Q], stats [Q][4], logs): results, counters and the candidate log in expansion order"""
    ids, d, st, logs = want
    assert np.array_equal(got["ids"], ids), what
    assert np.array_equal(_bits(got["d"]), _bits(d)), what
    assert np.array_equal(got["counters"], st), what
    assert np.array_equal(got["log_n"], st[:, 1]), what
    for i, log in enumerate(logs):
        assert np.array_equal(got["log"][i, :got["log_n"][i]], log[:got["log_n"][i]]), (what, i)


def _tiled_walk(trs, k, Q):
    ids, d, st, logs = S.from_traces(trs, k)
    return S.tile_want((ids, d, st), Q) + (S.tile_rows(logs, Q),)


# ---------------------------------------------------------------------------------------------------------------------
# the exact-distance family: narrow and wide builds, graph in HBM and pulled rows, fp16 rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,shape,L,k", S.EXACT_CASES, ids=S._ids(S.EXACT_CASES))
def test_exact(request, monkeypatch, family, name, shape, L, k):
    ix, q0 = S.load_input(name, request.getfixturevalue)
    q = S.tile(q0, NQ)
    _launch(monkeypatch, family, shape, L, NQ, dtype=ix.dtype)
    want = _tiled_walk(S.traces((family == "exact_f16", name), S.reference_index(family, ix), q0, L), k, NQ)
    with _engine(ix, S.FAMILIES[family].options) as e:
        got = _run(e, q, k, L)
        _check_walk(got, want, (family, name, shape, L))
        s = got["stats"]
        assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["rerank_fused"] == 0, s
        assert s["graph_pull"] == int("pull" in family or family == "exact_f16"), s
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# label filters: a second list of capacity L in every wave's slice
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,shape,L,k,extra", S.LABELS_CASES, ids=S._ids(S.LABELS_CASES))
def test_labels(request, monkeypatch, family, name, shape, L, k, extra):
    """rand4 labels and the `mixed` batch of tests/labels_inputs.py: neighbouring waves hold filtered and unfiltered queries"""
    ix, q0 = S.load_input(name, request.getfixturevalue)
    lanes = 2 if extra == "lanes2" else 1                                       # (bang_alloc runs a search kernel's batch in ONE lane whatever is asked)
    Q = NQ
    q = S.tile(q0, Q)
    excluded = X.make_mask("rand30", ix) if extra == "excluded" else None
    _launch(monkeypatch, family, shape, L, NQ, dtype=ix.dtype)
    trs = S.tile_rows(S.traces((False, name), ix, q0, L), Q)
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("mixed", Q)
    ids, d, matched, st, _ = LR.collect_all(trs, labels, any_, all_, k, L, int(ix.medoid), excluded)
    assert (matched[any_ != 0] < matched[any_ == 0].max()).any()               # (the filter bites)
    with _engine(ix, S.FAMILIES[family].options, lanes=lanes) as e:
        e.set_labels(labels)
        if excluded is not None:
            e.set_excluded(excluded)
        got = _run(e, q, k, L, filters=(any_, all_))
        _check_walk(got, (ids, d, st, [t.log for t in trs]), (family, name, shape, L, extra))
        assert np.array_equal(got["matched"], matched)
        s = got["stats"]
        assert s["label_launches"] == 1 and s["front_launches"] == 1 and s["exclude_launches"] == 0 and s["lanes"] == 1, s
        assert s["filtered_queries"] == int((any_ != 0).sum()), s
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# range search: radius, hit-log row and the hit count are per-query state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,shape,L,k,extra", S.RANGE_CASES, ids=S._ids(S.RANGE_CASES))
def test_range(request, monkeypatch, family, name, shape, L, k, extra):
    ix, q0 = S.load_input(name, request.getfixturevalue)
    lanes = 2 if extra == "lanes2" else 1                                       # (one lane all the same: see test_labels)
    Q = NQ
    q = S.tile(q0, Q)
    excluded = X.make_mask("rand30", ix) if extra == "excluded" else None
    _launch(monkeypatch, family, shape, L, NQ, dtype=ix.dtype)
    trs = S.tile_rows(S.range_traces(name, ix, q0, L), Q)
    walk = _tiled_walk(S.range_traces(name, ix, q0, L), L if excluded is not None else k, Q)
    if excluded is not None:                                                   # the top-k goes through bang_k_worklist_pick, as ever
        walk = X.worklist_all(walk[0], walk[1], excluded, k) + walk[2:]
    with _engine(ix, S.FAMILIES[family].options, lanes=lanes) as e:
        if excluded is not None:
            e.set_excluded(excluded)
        for rname, cap in S.RANGE_RADII:
            what = (family, name, shape, L, extra, rname, cap)
            radii = S.tile_rows(RI.radii(rname, S.range_reference(name, ix), ix, q0), Q)
            lims, hit_ids, hit_d, counts, offered = RR.collect_all(trs, radii, cap, excluded)
            if (rname, cap) == ("rank400", 64):
                assert (offered > cap).any()                                   # (the log is truncated)
            got = _run(e, q, k, L, radii=radii, cap=cap)
            _check_walk(got, walk, what)
            assert np.array_equal(got["offered"], offered) and np.array_equal(got["counts"], counts), what
            assert np.array_equal(got["lims"], lims), what
            assert np.array_equal(got["hit_ids"], hit_ids) and np.array_equal(_bits(got["hit_d"]), _bits(hit_d)), what
            s = got["stats"]
            assert s["range_launches"] == 1 and s["front_launches"] == 1 and s["range_queries"] == Q and s["lanes"] == 1, (what, s)
            assert s["range_truncated"] == int((offered > cap).sum()) and s["exclude_launches"] == (0 if excluded is None else 1), (what, s)
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the beam form: sixteen waves' worklists and survivor arrays at L = 512
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,beam", S.BEAM_CASES, ids=S._ids(S.BEAM_CASES))
def test_beam_longest_worklist(request, monkeypatch, family, beam):
    ix, q = S.tie_heavy32(request.getfixturevalue)
    L = S.MAX_L
    _launch(monkeypatch, family, "one_workgroup", L, NQ, dtype=ix.dtype, beam=beam)
    ids, d, st, log = S.beam_reference("tie_heavy", ix, q, L, beam)
    with _engine(ix, S.FAMILIES[family].options, beam=beam) as e:
        got = _run(e, q, L, L)
        _check_walk(got, (ids, d, st, list(log)), (family, beam))
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# search_kernel: every instance, the Inmemory build, the word-filter build, the LUT kernel
# ---------------------------------------------------------------------------------------------------------------------
def _check_pq(got, want, what):
    ids, d, st = got
    assert np.array_equal(ids, want[0]), what
    assert np.array_equal(_bits(d), _bits(want[1])), what
    assert np.array_equal(st, want[2]), what                                   # iterations, candidates, dist_evals, fetched


def _form(form, ix):
    return F.forms_of("self", ix.dtype, ix.D, ix.R, ix.N)[0] if form == "self" else form


def _search_cases(entries, forms):
    return [pytest.param(e, form, shape, L, id=f"{I.entry_id(e)}-{form}-{shape}-{L}") for e in entries for form in forms for shape, L in S.SEARCH_RUNS]


@pytest.mark.parametrize("entry,form,shape,L", _search_cases(I.ENTRIES, S.SEARCH_FORMS))
def test_search_kernel_instances(monkeypatch, entry, form, shape, L):
    ix, q0 = I.entry_index(entry)
    form = _form(form, ix)
    L = S.long_L(ix, entry.pq_ragged) if L == "long" else L
    k = 10
    q = S.tile(q0, NQ)
    _launch(monkeypatch, "search", shape, L, NQ, S.MIN_WAVES_SEARCH, pq=S.pq_args(ix, L, entry.pq_ragged))
    want = S.tile_want(S.oracle_reference(I.shape_of(entry), ix, q0, k, L), NQ)
    with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
        _check_pq(F.run(e, form, q, k, L), want, (I.entry_id(entry), form, shape, L))
        F.assert_form(e, form, ix, NQ, L, code_stride=I.stride_of(entry))
        e.free()
        e.unload()


# (semantics = 1 has no instance for 128-chunk code rows that are not dword-aligned: tests/test_gpu_search_instances.py asserts the refusal)
INMEMORY_ENTRIES = [e for e in I.ENTRIES if not (e.key == 132 and not I.aligned(e))]


@pytest.mark.parametrize("entry,form,shape,L", _search_cases(INMEMORY_ENTRIES, ("hbm",)))
def test_inmemory_build(monkeypatch, entry, form, shape, L):
    import edge_inputs as E
    ix, q0 = I.entry_index(entry)
    L = S.long_L(ix, entry.pq_ragged, inmemory=True) if L == "long" else L
    k = 10
    q = S.tile(q0, NQ)
    _launch(monkeypatch, "inmemory", shape, L, NQ, S.MIN_WAVES_SEARCH, pq=S.pq_args(ix, L, entry.pq_ragged))
    want = S.tile_want(E.first_k(S.inmemory_reference(I.shape_of(entry), ix, q0, L, L), k), NQ)
    with _engine(ix, S.FAMILIES["inmemory"].options, **I.options_of(entry)) as e:
        _check_pq(F.run(e, "self_fused", q, k, L), want, (I.entry_id(entry), shape, L))
        s = e.stats()
        assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["code_stride"] == I.stride_of(entry), s
        e.free()
        e.unload()


@pytest.mark.parametrize("shape,L", S.SEARCH_RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("form", ("self_fused", "pull_host"))
@pytest.mark.parametrize("name", list(WI.INPUTS))
def test_wordfilter_build(monkeypatch, name, form, shape, L):
    """The crafted queries of tests/wordfilter_inputs.py, where the word-local filter drops other ids than the split one, repeated to 32"""
    inp = WI.INPUTS[name]()
    ix, q0 = inp.ix, inp.q
    L = S.long_L(ix) if L == "long" else L
    k = 10
    q = S.tile(q0, NQ)
    _launch(monkeypatch, "wordfilter", shape, L, NQ, S.MIN_WAVES_SEARCH, pq=S.pq_args(ix, L))
    want = S.tile_want(S.wordfilter_reference(name, ix, q0, k, L), NQ)
    with F.open_engine(ix, form, monkeypatch, **S.FAMILIES["wordfilter"].options) as e:
        _check_pq(F.run(e, form, q, k, L), want, (name, form, shape, L))
        assert F.assert_form(e, form, ix, NQ, L)["filter_layout"] == 1
        e.free()
        e.unload()


@pytest.mark.parametrize("name", S.LUT_INPUTS)
def test_lut_kernel_longest_worklist(request, monkeypatch, name):
    ix, q0 = S.load_input(name, request.getfixturevalue)
    L, k = S.MAX_L, 10
    q = S.tile(q0, NQ)
    _launch(monkeypatch, "lut", "one_workgroup", L, NQ)
    want = S.tile_want(S.oracle_reference(name, ix, q0, k, L), NQ)
    with _engine(ix, S.FAMILIES["lut"].options, **(dict(pq=1) if name in S.NARROW else {})) as e:
        _check_pq(F.run(e, "lut_kernel", q, k, L), want, name)
        F.assert_form(e, "lut_kernel", ix, NQ, L)
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the whole chip in full workgroups: the branch of the geometry that a benchmark batch takes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name", S.FULL_CASES, ids=S._ids(S.FULL_CASES))
def test_full_chip(request, monkeypatch, family, name):
    ix, q0 = S.load_input(name, request.getfixturevalue)
    L, k = S.FULL_L, S.FULL_K
    fam = S.FAMILIES[family]
    kw = {}
    if fam.kind in ("search", "search8"):
        kw["pq"] = S.pq_args(ix, L)
    elif fam.kind != "lut":
        kw["dtype"] = ix.dtype
    if family == "beam":
        kw["beam"] = S.FULL_BEAM
    Q, full = S.full_chip_batch(family, L, **kw)
    S.set_caps(monkeypatch, "full_chip")
    S.assert_reached("full_chip", S.geometry(family, L, Q, "full_chip", **kw), Q, full,
                     S.MIN_WAVES_SEARCH if fam.kind in ("search", "search8") else S.MIN_WAVES, S.rounds_of(family))
    q = S.tile(q0, Q)
    what = (family, name, Q, full)
    if fam.kind in ("search", "search8"):
        form = "self_fused"
        if family == "search":
            want = S.oracle_reference(name, ix, q0, k, L)
        elif family == "inmemory":
            want = S.inmemory_reference(name, ix, q0, k, L)
        else:
            want = S.wordfilter_reference(name, ix, q0, k, L)
        options = F.OPTIONS[form] if fam.options is None else dict(F.OPTIONS[form], **fam.options)
        with _engine(ix, options) as e:
            _check_pq(F.run(e, form, q, k, L), S.tile_want(want, Q), what)
            assert e.stats()["search_kernel"] == 1 and e.stats()["front_launches"] == 1
            e.free()                                                           # (a visited filter per query: given back here)
            e.unload()
        return
    with _engine(ix, fam.options, **(dict(beam=S.FULL_BEAM) if family == "beam" else {})) as e:
        if family == "beam":
            ids, d, st, log = S.beam_reference(name, ix, q0, L, S.FULL_BEAM)
            want = S.tile_want((np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(d[:k]), st), Q) + (S.tile_rows(list(log), Q),)
            _check_walk(_run(e, q, k, L), want, what)
        elif family == "labels":
            trs = S.traces((False, name), ix, q0, L)
            labels = LI.rand4(ix.N)
            any_, all_ = LI.batch("mixed", NQ)                                 # (a copy of a query carries the filter of the original)
            ids, d, matched, st, _ = LR.collect_all(trs, labels, any_, all_, k, L, int(ix.medoid))
            e.set_labels(labels)
            got = _run(e, q, k, L, filters=(S.tile_rows(any_, Q), S.tile_rows(all_, Q)))
            _check_walk(got, S.tile_want((ids, d, st), Q) + (S.tile_rows([t.log for t in trs], Q),), what)
            assert np.array_equal(got["matched"], S.tile_rows(matched, Q))
        elif family == "range":
            rname, cap = S.FULL_RANGE
            trs = S.range_traces(name, ix, q0, L)
            radii = RI.radii(rname, S.range_reference(name, ix), ix, q0)
            lims, hit_ids, hit_d, counts, offered = RR.collect_all(S.tile_rows(trs, Q), S.tile_rows(radii, Q), cap)
            got = _run(e, q, k, L, radii=S.tile_rows(radii, Q), cap=cap)
            _check_walk(got, _tiled_walk(trs, k, Q), what)
            assert np.array_equal(got["offered"], offered) and np.array_equal(got["counts"], counts) and np.array_equal(got["lims"], lims), what
            assert np.array_equal(got["hit_ids"], hit_ids) and np.array_equal(_bits(got["hit_d"]), _bits(hit_d)), what
        else:
            trs = S.traces((family == "exact_f16", name), S.reference_index(family, ix), q0, L)
            _check_walk(_run(e, q, k, L), _tiled_walk(trs, k, Q), what)
        s = e.stats()
        assert s["search_kernel"] == 1 and s["front_launches"] == 1, s
        e.unload()                                                             # (_run freed the allocation: a visited filter per query)


# ---------------------------------------------------------------------------------------------------------------------
# a launch that is a sub-range of a larger batch: rr_q0 != 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("exact", "labels", "range"))
def test_sub_range_of_a_larger_batch(small_u8, kind):
    """The kernels index the launch's own arrays (visited filter, candidate log, counters) by q and the batch's arrays (queries, results, filters,
    matched, radii, hit log, offered) by rr_q0 + q.  The engine runs a search kernel's batch in one lane, so through it rr_q0 is always 0: here the
    entry points are called directly for rows 5 .. 36 of a batch of 40, in one full workgroup.  The rows outside the launch hold other queries,
    filters that match nobody and infinite radii, and their outputs must stay as they were."""
    import ctypes as C
    from bang_amd import binding as B
    ix, qs = small_u8[:2]
    Q0, Q, Qt, k, L, cap = 5, NQ, NQ + 8, 10, 37, 64
    q = np.ascontiguousarray(qs[:Q])
    family = {"exact": "exact", "labels": "labels", "range": "range"}[kind]
    full = S.geometry(family, L, S.FULL_Q, "full_chip", dtype=ix.dtype)
    S.assert_reached("one_workgroup", S.geometry(family, L, Q, "one_workgroup", dtype=ix.dtype), Q, full)
    allq = np.ascontiguousarray(np.concatenate([qs[Q:Q + Q0], q, qs[Q + Q0:Q + Qt - Q]]))
    assert allq.shape[0] == Qt
    trs = S.traces((False, "small_u8"), ix, q, L)
    adj = ix.adjacency()[ix.medoid][: int(ix.degrees()[ix.medoid])]
    seed = np.zeros(2 + 65, dtype=np.uint32)
    seed[0], seed[1] = 1 + len(adj), ix.medoid
    seed[2:2 + len(adj)] = adj
    MARK = 0xA5A5A5A5
    ids0 = np.full((Qt, k), MARK, np.uint64)
    d0 = np.full((k, Qt), MARK, np.uint32)
    buf = dict(seed=B.DeviceBuffer.from_numpy(seed), graph=B.DeviceBuffer.from_numpy(ix.graph, slack=256), q=B.DeviceBuffer.from_numpy(allq, slack=16),
               bloom=B.DeviceBuffer(Q * B.BF_WORDS * 4), cand=B.DeviceBuffer(Q * (L + 50) * 4), cnt=B.DeviceBuffer(Q * 4), qstats=B.DeviceBuffer(Q * 8),
               iters=B.DeviceBuffer(Q * 4), ctl=B.DeviceBuffer(64), ids=B.DeviceBuffer.from_numpy(ids0), dists=B.DeviceBuffer.from_numpy(d0))
    try:
        sp = B.SearchParams()
        sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter, sp.max_wgs = Q, ix.R, L, ix.medoid, L + 49, 1
        sp.d_seed, sp.d_graph, sp.entry_len, sp.vec_bytes, sp.n_nodes = buf["seed"].ptr, buf["graph"].ptr, ix.entry_len, ix.D, ix.N
        sp.d_bloom, sp.d_cand_ids, sp.d_cand_cnt, sp.d_qstats, sp.d_qiters = buf["bloom"].ptr, buf["cand"].ptr, buf["cnt"].ptr, buf["qstats"].ptr, buf["iters"].ptr
        sp.d_next_query, sp.d_abort = buf["ctl"].ptr, buf["ctl"].ptr + 4
        sp.rr_queries, sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = buf["q"].ptr, B.DTYPE_CODE[ix.dtype], ix.D, k, Q0, Qt
        sp.rr_ids_out, sp.rr_dists_out = buf["ids"].ptr, buf["dists"].ptr
        lib = B.lib()
        want_ids, want_d, st, logs = S.from_traces(trs, k)
        if kind == "exact":
            f = lib.bang_k_search_exact
            f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
            assert f(C.byref(sp), None) == 0, lib.bang_last_error().decode()
        elif kind == "labels":
            labels = LI.rand4(ix.N)
            any_, all_ = LI.batch("mixed", Q)
            filt = np.full((Qt, 2), 0xFFFFFFFF, np.uint32)                     # (outside the launch: filters that match nobody)
            filt[Q0:Q0 + Q, 0], filt[Q0:Q0 + Q, 1] = any_, all_
            buf.update(labels=B.DeviceBuffer.from_numpy(labels), filt=B.DeviceBuffer.from_numpy(filt),
                       matched=B.DeviceBuffer.from_numpy(np.full(Qt, MARK, np.uint32)))
            lf = B.LabelFilter()
            lf.d_labels, lf.d_filters, lf.d_excluded, lf.d_matched = buf["labels"].ptr, buf["filt"].ptr, None, buf["matched"].ptr
            f = lib.bang_k_search_exact_labels
            f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
            assert f(C.byref(sp), C.byref(lf), None) == 0, lib.bang_last_error().decode()
            want_ids, want_d, matched, _, _ = LR.collect_all(trs, labels, any_, all_, k, L, int(ix.medoid))
        else:
            radii = RI.radii("mixed", S.range_reference("small_u8", ix), ix, q)
            rad = np.full(Qt, np.inf, np.float32)                              # (outside the launch: every evaluated node)
            rad[Q0:Q0 + Q] = radii
            buf.update(rad=B.DeviceBuffer.from_numpy(rad), hit_ids=B.DeviceBuffer.from_numpy(np.full((Qt, cap), MARK, np.uint32)),
                       hit_d=B.DeviceBuffer.from_numpy(np.full((Qt, cap), MARK, np.uint32)), offered=B.DeviceBuffer.from_numpy(np.full(Qt, MARK, np.uint32)))
            ro = B.RangeOut()
            ro.d_radius, ro.d_excluded, ro.d_hit_ids, ro.d_hit_dists, ro.d_offered, ro.cap = (buf["rad"].ptr, None, buf["hit_ids"].ptr, buf["hit_d"].ptr,
                                                                                              buf["offered"].ptr, cap)
            f = lib.bang_k_search_exact_range
            f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
            assert f(C.byref(sp), C.byref(ro), None) == 0, lib.bang_last_error().decode()
        B.sync()
        assert int(buf["ctl"].download(np.uint32, (2,))[1]) == 0               # no id out of range
        ids = buf["ids"].download(np.uint64, (Qt, k))
        d = buf["dists"].download(np.uint32, (k, Qt))
        inside = np.zeros(Qt, bool)
        inside[Q0:Q0 + Q] = True
        assert np.array_equal(ids[inside], want_ids) and np.array_equal(d[:, inside], _bits(want_d))
        assert (ids[~inside] == MARK).all() and (d[:, ~inside] == MARK).all()  # the other rows of the batch are not this launch's
        cnt = buf["cnt"].download(np.uint32, (Q,))
        log = buf["cand"].download(np.uint32, (Q, L + 50))
        qst = buf["qstats"].download(np.uint32, (Q, 2))
        assert np.array_equal(buf["iters"].download(np.uint32, (Q,)), st[:, 0]) and np.array_equal(cnt, st[:, 1])
        assert np.array_equal(qst[:, 0], st[:, 2]) and np.array_equal(qst[:, 1], st[:, 3])
        for i in range(Q):
            assert np.array_equal(log[i, :cnt[i]], logs[i]), i
        if kind == "labels":
            m = buf["matched"].download(np.uint32, (Qt,))
            assert np.array_equal(m[inside], matched) and (m[~inside] == MARK).all()
        if kind == "range":
            offered = buf["offered"].download(np.uint32, (Qt,))
            hit_ids = buf["hit_ids"].download(np.uint32, (Qt, cap))
            hit_d = buf["hit_d"].download(np.uint32, (Qt, cap))
            assert (offered[~inside] == MARK).all() and (hit_ids[~inside] == MARK).all() and (hit_d[~inside] == MARK).all()
            rtr = S.range_traces("small_u8", ix, q, L)
            for i in range(Q):                                                 # the raw log: every hit in evaluation order, the first `cap` kept
                h_ids, h_d, _ = RR.hits(rtr[i], radii[i])
                n = min(len(h_ids), cap)
                assert int(offered[Q0 + i]) == len(h_ids), i
                assert np.array_equal(hit_ids[Q0 + i, :n], h_ids[:n]) and np.array_equal(hit_d[Q0 + i, :n], _bits(h_d[:n])), i
                assert (hit_ids[Q0 + i, n:] == MARK).all(), i
            assert (offered[inside] > cap).any() and (offered[inside] == 0).any()
    finally:
        for b in buf.values():
            b.free()
