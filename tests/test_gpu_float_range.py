"""Float data at the ends of the float range (tests/float_range_inputs.py: scaled by 2^+-46, scaled until the distances are subnormal, until they
are all +0, shifted by -128 with -0.0 and bit-copies, shifted by 2^20) through every kernel family that reads float data, against that family's
CPU reference on the same index, bit for bit: ids, distance bits, the per-query counters, and the candidate log where the family's own tests
compare it.  The contract "the explicit fmaf chain, same bits on CPU and GPU" depends on the code object's denormal mode and on no kernel taking
a shortcut that is exact for moderate magnitudes only; every other float input of the suite has elements of magnitude 0.3.  The exact families
are held to plain arithmetic as well: |d - d64| <= (D + 2) 2^-24 d64 against the float64 squared L2 of the float32 inputs -- the bound for D
rounded differences accumulated through D fused multiply-adds -- which checks kernel and reference together.  tests/test_float_range_inputs.py
asserts without a GPU that every input reaches the edge it is named for, that 2^+-46 leaves ids, counters and logs of every reference unchanged
and shifts every distance's exponent, and that every evaluated distance stays finite and below the padding sentinel.

Then the refusals (CANON 20): a NaN, +-inf or 2^57 in a query batch, a NaN in the pivot table or the vectors of an index.
They return before any launch -- no test here passes a value outside the domain to a kernel."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import base_forms as F
import float_range_inputs as FR
import fp16_inputs as FP
import instance_inputs as I
import labels_inputs as LI
import labels_reference as LR
import range_inputs as RI
import range_reference as RR
from beam_reference import Reference as BeamReference
from exact_reference import Reference as ExactReference
from inmemory_reference import Reference as InmemReference
from wordfilter_reference import Reference as WordReference

pytestmark = pytest.mark.gpu

K = FR.K
LS = FR.LS
CAP = 512
PQ_BASES = ("d68", "d4")                       # layouts with a search-kernel instance
LUT_BASES = ("d252", "f32_260")                # layouts on the LUT path
NARROW = ("d68", "d4", "d252")                 # the exact-distance kernel's narrow instances;  f32_260: the wide ones
PQ_GROUPS = {"self": ("self_fused", "self_launch"), "pulled": ("pull_host", "pull_hbm"), "host_paced": ("walker_graph", "walker_rows"), "loop": ("loop",)}
EXACT_FORMS = {"hbm": dict(graph=1, distance=1), "pull": dict(graph=0, pull=1, distance=1)}
FP16_INPUTS = ("fp16_straddle", "signed")      # (2^20 and 2^46 leave fp16's range, 2^-46 and below its subnormals)
FP16_RERANK = {"pull": dict(pull=1), "loop": dict(persistent=0, vectors=1)}
ACCURACY = ("up", "down", "signed", "offset")
_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle(base, what, L, mips=False):
    from oracle import oracle as O
    ix, q = FR.get(base, what)
    qq = np.ascontiguousarray(q[:, :-1]) if mips else q       # MIPS: the queries carry D - 1 coordinates
    return _cached(("oracle", base, what, L, mips), lambda: O.Oracle(ix).search(qq, K, L, mips=mips, with_stats=True))


def _exact(base, what, L):
    ix, q = FR.get(base, what)
    return _cached(("exact", base, what, L), lambda: ExactReference(ix).search(q, K, L, "exact"))


def _run(e, q, k, L, distfn=0):
    e.set_searchparams(k, L, distfn)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    return ids, d, e.query_counters(q.shape[0])


def _params(bases, inputs, *more):
    out = []
    for b in bases:
        for w in inputs:
            for m in (more[0] if more else [None]):
                rest = () if m is None else (m,)
                out.append(pytest.param(b, w, *rest, id="-".join([b, w] + [str(x) for x in rest])))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the PQ walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,what,group", _params(PQ_BASES, FR.NAMES, tuple(PQ_GROUPS)))
def test_pq_walk_in_every_form(base, what, group, monkeypatch):
    """self_fused, self_launch / pull_host, pull_hbm / walker_graph, walker_rows / loop.  The host-paced forms skip exactly as base_forms.run does."""
    ix, q = FR.get(base, what)
    assert F.fusable(ix.dtype, ix.D, ix.entry_len)
    for form in PQ_GROUPS[group]:
        with F.open_engine(ix, form, monkeypatch) as e:
            for L in LS:
                F.assert_same(F.run(e, form, q, K, L), _oracle(base, what, L), form)
                F.assert_form(e, form, ix, q.shape[0], L)
                e.free()
            e.unload()


@pytest.mark.parametrize("base,what,form", _params(LUT_BASES, FR.NAMES, F.LUT_FORMS))
def test_pq_walk_on_the_lut_path(base, what, form, monkeypatch):
    ix, q = FR.get(base, what)
    with F.open_engine(ix, form, monkeypatch) as e:
        for L in LS:
            F.assert_same(F.run(e, form, q, K, L), _oracle(base, what, L), form)
            F.assert_form(e, form, ix, q.shape[0], L)
            e.free()
        e.unload()


@pytest.mark.parametrize("base,what,form", _params(("d68",), FR.NAMES, ("self_fused", "loop")))
def test_pq_walk_mips(base, what, form, monkeypatch):
    ix, q = FR.get(base, what)
    q1 = np.ascontiguousarray(q[:, :-1])                      # MIPS: the queries carry D - 1 coordinates
    with F.open_engine(ix, form, monkeypatch) as e:
        for L in LS:
            F.assert_same(_run(e, q1, K, L, distfn=1), _oracle(base, what, L, mips=True), form)
            assert e.stats()["search_kernel"] == int(form == "self_fused")
            e.free()
        e.unload()


@pytest.mark.parametrize("base,what", _params(PQ_BASES, FR.NAMES))
def test_inmemory_semantics(base, what):
    import bang_amd
    ix, q = FR.get(base, what)
    with bang_amd.Engine(ix.dtype, graph=1, semantics=1) as e:
        e.load_index(ix)
        for L in LS:
            want = _cached(("inmemory", base, what, L), lambda: InmemReference(ix).search(q, K, L, "inmemory"))
            F.assert_same(_run(e, q, K, L), want)
            s = e.stats()
            assert s["search_kernel"] == 1 and s["front_launches"] == 1, s
            e.free()
        e.unload()


@pytest.mark.parametrize("base,what", _params(PQ_BASES, FR.NAMES))
def test_word_filter_layout(base, what, monkeypatch):
    ix, q = FR.get(base, what)
    with F.open_engine(ix, "self_fused", monkeypatch, filter_layout=1) as e:
        for L in LS:
            want = _cached(("word", base, what, L), lambda: WordReference(ix).search(q, K, L, "word"))
            F.assert_same(_run(e, q, K, L), want)
            s = e.stats()
            assert s["filter_layout"] == 1 and s["search_kernel"] == 1, s
            e.free()
        e.unload()


@pytest.mark.parametrize("what", FP16_INPUTS)
@pytest.mark.parametrize("form", list(FP16_RERANK))
def test_rerank_over_an_fp16_table(form, what):
    """The vector table holds normal and subnormal halves side by side (fp16_straddle) / values of both kinds of zero and magnitude 128 (signed):
    the expected bits are the oracle's on the index rounded to fp16 (fp16_inputs.rounded)."""
    import bang_amd
    ix, q = FR.get("fp16_256", what)
    rounded = _cached(("rounded", what), lambda: FP.rounded(ix))
    with bang_amd.Engine(ix.dtype, graph=0, vectors_fp16=1, **FP16_RERANK[form]) as e:
        e.load_index(ix)
        for L in LS:
            want = FP.pq_reference(("float_range", what), rounded, q, K, L)
            ids, d, st = _run(e, q, K, L)
            assert np.array_equal(ids, want[0]) and np.array_equal(_bits(d), _bits(want[1]))
            s = e.stats()
            assert s["vectors_fp16"] == 1 and s["vector_table_bytes"] == FP.table_bytes(ix.N, ix.D), s
            assert np.array_equal(st if s["search_kernel"] else st[:, 1:], want[2] if s["search_kernel"] else want[2][:, 1:])
            e.free()
        e.unload()


@pytest.mark.parametrize("entry", [x for x in I.ENTRIES if x.dtype == "float"], ids=I.entry_id)
@pytest.mark.parametrize("scale", ("down", "subnormal"))
def test_search_kernel_instances(entry, scale, monkeypatch):
    """Every float entry of tests/instance_inputs.py once at 2^-46 and once with subnormal distances, in the self-paced form with the fused re-rank."""
    from oracle import oracle as O
    ix0, q0 = I.entry_index(entry)
    e_ = FR.DOWN_EXP if scale == "down" else FR.exps_of(ix0, q0)[0]
    ix, q = FR.scaled(ix0, q0, e_)
    form = "self_fused"                                        # (a layout the fused re-rank does not evaluate runs the re-rank launch: assert_form)
    L = 37
    want = _cached(("instance", I.shape_of(entry), scale), lambda: O.Oracle(ix).search(q, K, L, with_stats=True))
    if scale == "subnormal":
        assert FR.is_subnormal(FR.top10_exact(ix, q)).mean() >= 0.5
    with F.open_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
        F.assert_same(F.run(e, form, q, K, L), want, form)
        F.assert_form(e, form, ix, q.shape[0], L, code_stride=I.stride_of(entry))
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# distance = 1
# ---------------------------------------------------------------------------------------------------------------------
def _assert_accuracy(ix, q, ids, d):
    """|d - d64| <= (D + 2) 2^-24 d64 for every returned (id, distance): plain float64 arithmetic on the float32 inputs."""
    v = ix.vectors().astype(np.float64)
    bound = (ix.D + 2) * 2.0 ** -24
    for i in range(q.shape[0]):
        real = ids[i] != np.iinfo(np.uint64).max
        d64 = ((v[ids[i][real].astype(np.int64)] - q[i].astype(np.float64)[None, :]) ** 2).sum(axis=1)
        got = d[:, i][real].astype(np.float64)
        assert (np.abs(got - d64) <= bound * d64).all(), (i, got, d64)


@pytest.mark.parametrize("base,what,form", _params(NARROW + ("f32_260",), FR.NAMES, tuple(EXACT_FORMS)))
def test_exact_distance_walk(base, what, form):
    """exact, exact_pull on the narrow layouts; exact_wide, exact_wide_pull on f32_260."""
    import bang_amd
    ix, q = FR.get(base, what)
    with bang_amd.Engine(ix.dtype, **EXACT_FORMS[form]) as e:
        e.load_index(ix)
        for L in LS:
            got = _run(e, q, K, L)
            F.assert_same(got, _exact(base, what, L))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["rerank_fused"] == 0 and s["graph_pull"] == int(form == "pull"), s
            if what in ACCURACY:
                _assert_accuracy(ix, q, got[0], got[1])
            e.free()
        e.unload()


@pytest.mark.parametrize("what", FP16_INPUTS)
def test_exact_distance_walk_on_an_fp16_table(what):
    import bang_amd
    ix, q = FR.get("fp16_256", what)
    rounded = _cached(("rounded", what), lambda: FP.rounded(ix))
    with bang_amd.Engine(ix.dtype, graph=0, pull=1, distance=1, vectors_fp16=1) as e:
        e.load_index(ix)
        for L in LS:
            got = _run(e, q, K, L)
            F.assert_same(got, FP.exact_reference(("float_range", what), rounded, q, K, L))
            s = e.stats()
            assert s["vectors_fp16"] == 1 and s["search_kernel"] == 1 and s["graph_pull"] == 1, s
            _assert_accuracy(rounded, q, got[0], got[1])
            e.free()
        e.unload()


@pytest.mark.parametrize("base,what,form", _params(("d68", "d252"), FR.NAMES, tuple(EXACT_FORMS)))
@pytest.mark.parametrize("W", (2, 4))
def test_beam(W, base, what, form):
    import bang_amd
    ix, q = FR.get(base, what)
    Q = q.shape[0]
    with bang_amd.Engine(ix.dtype, beam=W, **EXACT_FORMS[form]) as e:
        e.load_index(ix)
        for L in LS:
            ids_r, d_r, st_r, log_r = _cached(("beam", base, what, L, W), lambda: BeamReference(ix).search(q, K, L, W))
            got = _run(e, q, K, L)
            F.assert_same(got, (ids_r, d_r, st_r))
            log, cnt = e.candidate_log(Q, L)
            assert np.array_equal(cnt, st_r[:, 1])
            for i in range(Q):
                assert np.array_equal(log[i, :cnt[i]], log_r[i, :cnt[i]]), i
            if what in ACCURACY:
                _assert_accuracy(ix, q, got[0], got[1])
            e.free()
        e.unload()


@pytest.mark.parametrize("base,what,form", _params(("d68", "d252"), FR.NAMES, tuple(EXACT_FORMS)))
def test_label_filters(base, what, form):
    """labels_inputs.rand4 and the selective batch all2 (two tags at once: about one node in eight matches)."""
    import bang_amd
    ix, q = FR.get(base, what)
    Q = q.shape[0]
    labels = LI.rand4(ix.N)
    any_, all_ = LI.batch("all2", Q)
    with bang_amd.Engine(ix.dtype, **EXACT_FORMS[form]) as e:
        e.load_index(ix)
        e.set_labels(labels)
        for L in LS:
            tr = _cached(("walks", base, what, L), lambda: LR.Reference(ix).walks(q, L))
            ids_r, d_r, matched_r, st_r, _ = LR.collect_all(tr, labels, any_, all_, K, L, int(ix.medoid))
            e.set_searchparams(K, L)
            e.alloc(Q)
            e.set_filters(any_, all_)
            e.init(Q)
            ids, d = e.query(q)
            F.assert_same((ids, d, e.query_counters(Q)), (ids_r, d_r, st_r))
            assert np.array_equal(e.matched_counts(Q), matched_r)
            log, cnt = e.candidate_log(Q, L)
            for i, t in enumerate(tr):
                assert np.array_equal(log[i, :cnt[i]], t.log), i
            s = e.stats()
            assert s["label_launches"] == 1 and s["front_launches"] == 1 and s["filtered_queries"] == Q, s
            if what in ACCURACY:
                _assert_accuracy(ix, q, ids, d)
            e.free()
        e.unload()


def _radii(base, what, ix, q):
    """rank100 computed on THIS index (at `subnormal` a subnormal radius on the `<=` edge of every query); +inf; +0.0 and -0.0 where distances of
    zero exist."""
    Q = q.shape[0]
    out = [("rank100", RI.radii("rank100", ExactReference(ix), ix, q)), ("inf", np.full(Q, np.inf, np.float32))]
    if what in ("zero", "signed"):
        out += [("+0", np.full(Q, 0.0, np.float32)), ("-0", np.full(Q, -0.0, np.float32))]
    return out


@pytest.mark.parametrize("base,what,form", _params(("d68", "d252"), FR.NAMES, tuple(EXACT_FORMS)))
def test_range_search(base, what, form):
    import bang_amd
    ix, q = FR.get(base, what)
    Q = q.shape[0]
    radii = _cached(("radii", base, what), lambda: _radii(base, what, ix, q))
    if what == "subnormal":
        assert FR.is_subnormal(radii[0][1]).mean() >= 0.5
    with bang_amd.Engine(ix.dtype, range_hits=CAP, **EXACT_FORMS[form]) as e:
        e.load_index(ix)
        for L in LS:
            tr = _cached(("traces", base, what, L), lambda: RR.Reference(ix).evaluated_all(q, L))
            for label, r in radii:
                e.set_searchparams(K, L)
                e.alloc(Q)
                e.set_radii(r)
                e.init(Q)
                ids, d = e.query(q)
                F.assert_same((ids, d, e.query_counters(Q)), _exact(base, what, L))
                lims_r, ids_r, d_r, counts_r, offered_r = RR.collect_all(tr, r, CAP)
                counts, offered = e.range_counts(Q)
                lims, hit_ids, hit_d = e.range_results(Q)
                assert np.array_equal(offered, offered_r) and np.array_equal(counts, counts_r) and np.array_equal(lims, lims_r), (L, label)
                assert np.array_equal(hit_ids, ids_r) and np.array_equal(_bits(hit_d), _bits(d_r)), (L, label)
                log, cnt = e.candidate_log(Q, L)
                for i, t in enumerate(tr):
                    assert np.array_equal(log[i, :cnt[i]], t.log), i
                s = e.stats()
                assert s["range_launches"] == 1 and s["front_launches"] == 1 and s["range_queries"] == Q, s
                if label == "rank100":
                    assert counts.sum() > 0
                if label in ("+0", "-0"):
                    assert counts[0] > 0                                                  # (a distance of +0 is within a radius of -0)
                e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# refusals: nothing below reaches a kernel with a value outside the domain
# ---------------------------------------------------------------------------------------------------------------------
REFUSAL_ENGINES = {"pq_hbm": dict(graph=1), "exact_hbm": dict(graph=1, distance=1), "pq_pull": dict(graph=0, pull=1)}
BAD_VALUES = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "2^57": np.float32(2.0 ** 57)}
FILL = 0xAB


@pytest.mark.parametrize("engine", list(REFUSAL_ENGINES))
def test_a_batch_outside_the_domain_is_refused_before_any_launch(engine):
    import bang_amd
    from bang_amd import binding as B
    ix, q = FR.get("d68", "unscaled")
    Q, D, L = q.shape[0], ix.D, 37
    want = _exact("d68", "unscaled", L) if engine == "exact_hbm" else _oracle("d68", "unscaled", L)
    d_ids, d_d = B.DeviceBuffer(Q * K * 8), B.DeviceBuffer(K * Q * 4)
    try:
        with bang_amd.Engine(ix.dtype, **REFUSAL_ENGINES[engine]) as e:
            e.load_index(ix)
            e.set_searchparams(K, L)
            e.alloc(Q)
            e.init(Q)
            ids, d = e.query(q)
            F.assert_same((ids, d, e.query_counters(Q)), want)
            for name, v in BAD_VALUES.items():
                for qi, dim in ((0, 3), (Q - 1, 0), (Q // 2, D - 1)):
                    bad = q.copy()
                    bad[qi, dim] = v
                    if qi == 0:
                        bad[Q - 1, 5] = np.float32(np.nan)                                # a later offender: the first one is named
                    e.init(Q)
                    before, counters = e.stats(), e.query_counters(Q)
                    for buf in (d_ids, d_d):
                        B._check(B.lib().bang_dev_memset(C.c_void_p(buf.ptr), FILL, C.c_size_t(buf.nbytes)), "bang_dev_memset")
                    msg = rf"query {qi}, dimension {dim} "
                    with pytest.raises(bang_amd.BangError, match=msg):
                        e.query(bad)
                    with pytest.raises(bang_amd.BangError, match=msg):
                        e.query_dev(bad, d_ids.ptr, d_d.ptr)
                    B.sync()
                    assert e.stats() == before and np.array_equal(e.query_counters(Q), counters), (name, qi, dim)
                    assert (d_ids.download(np.uint8, (d_ids.nbytes,)) == FILL).all() and (d_d.download(np.uint8, (d_d.nbytes,)) == FILL).all()
                    ids, d = e.query(q)                                                   # the same allocation, the state bang_init left: the clean batch
                    F.assert_same((ids, d, e.query_counters(Q)), want)
            e.free()
            e.unload()
    finally:
        d_ids.free()
        d_d.free()


def test_a_mips_batch_is_checked_at_its_own_row_length():
    """MIPS queries carry D - 1 coordinates: the check reads Q x (D - 1) floats -- a NaN right behind the batch is not its business -- and names
    query and dimension by that row length."""
    import bang_amd
    ix, q = FR.get("d68", "unscaled")
    Q, D, L = q.shape[0], ix.D, 37
    buf = np.full(Q * (D - 1) + D, np.nan, np.float32)
    buf[:Q * (D - 1)] = q[:, :-1].reshape(-1)
    q1 = buf[:Q * (D - 1)].reshape(Q, D - 1)                                              # a view: the NaNs lie behind it in memory
    want = _oracle("d68", "unscaled", L, mips=True)
    with bang_amd.Engine(ix.dtype, graph=1) as e:
        e.load_index(ix)
        assert np.shares_memory(np.ascontiguousarray(q1, np.float32), buf)                # (what Engine.query hands over is that view, not a copy)
        ids, d, _ = _run(e, q1, K, L, distfn=1)
        F.assert_same((ids, d, e.query_counters(Q)), want)
        bad = q1.copy()
        bad[Q - 1, D - 2] = np.float32(np.inf)
        e.init(Q)
        with pytest.raises(bang_amd.BangError, match=rf"query {Q - 1}, dimension {D - 2} "):
            e.query(bad)
        ids, d = e.query(q1)
        F.assert_same((ids, d, e.query_counters(Q)), want)
        e.free()
        e.unload()


def _write_files_unchecked(prefix, ix):
    """formats.write_index without its check: the four files as they are."""
    from bang_amd import formats
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    formats.write_pq_pivots(prefix + formats.PQ_PIVOTS_SUFFIX, ix.pivots, ix.centroid, ix.chunk_off)
    formats.write_pq_compressed(prefix + formats.PQ_COMPRESSED_SUFFIX, ix.codes)
    with open(prefix + formats.GRAPH_SUFFIX, "wb") as f:
        f.write(np.ascontiguousarray(ix.graph).tobytes())
    formats.write_graph_metadata(prefix + formats.GRAPH_META_SUFFIX, ix.medoid, ix.entry_len, ix.dtype, ix.D, ix.R, ix.N)


@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_an_index_with_a_nan_pivot_is_refused(fixture, request, tmp_path):
    """dtype uint8 and float: Engine.load_index (numpy), bang_load_mem_e (the library's own check) and bang_load on index files."""
    import bang_amd
    from bang_amd import binding as B, formats
    ix = request.getfixturevalue(fixture)[0]
    piv = ix.pivots.copy()
    piv[200, ix.D - 1] = np.nan
    bad = dataclasses.replace(ix, pivots=piv)
    cen = ix.centroid.copy()
    cen[1] = -np.inf
    for graph in (0, 1):
        with bang_amd.Engine(ix.dtype, graph=graph) as e:
            with pytest.raises(bang_amd.BangError, match=r"pivot.*\(200, %d\)" % (ix.D - 1)):
                e.load_index(bad)
            with pytest.raises(bang_amd.BangError, match="centroid"):
                e.load_index(dataclasses.replace(ix, centroid=cen))
            # the library's check, without the binding's in front of it
            keep = [np.ascontiguousarray(a) for a in (ix.graph, ix.codes, piv, ix.centroid, ix.chunk_off)]
            d = B.IndexDesc(ix.medoid, ix.entry_len, ix.D, ix.R, ix.N, ix.m, *[B._vp(a).value for a in keep[:2]], None, *[B._vp(a).value for a in keep[2:]], 0)
            assert B.lib().bang_load_mem_e(e._h, C.byref(d)) == -1
            assert f"pivot 200, dimension {ix.D - 1}" in B.lib().bang_last_error().decode()
            prefix = str(tmp_path / f"g{graph}" / "ix")
            _write_files_unchecked(prefix, bad)
            with pytest.raises(bang_amd.BangError, match=rf"pivot 200, dimension {ix.D - 1} "):
                e.load(prefix)
            e.load_index(ix)                                                             # the engine is still usable
            e.unload()
    with pytest.raises(ValueError, match="pivot"):
        formats.write_index(str(tmp_path / "w" / "ix"), bad)


def test_an_index_with_a_nan_vector_element_is_refused(small_f32, tmp_path):
    import bang_amd
    from bang_amd import formats
    ix = small_f32[0]
    g = ix.graph.copy()
    g[ix.N - 1, 4 * (ix.D - 1): 4 * ix.D] = np.array([np.nan], np.float32).view(np.uint8)
    bad = dataclasses.replace(ix, graph=g)
    with bang_amd.Engine(ix.dtype, graph=1) as e:
        with pytest.raises(bang_amd.BangError, match=r"vectors: element \(%d, %d\)" % (ix.N - 1, ix.D - 1)):
            e.load_index(bad)
    with pytest.raises(ValueError, match="vectors"):
        formats.write_index(str(tmp_path / "w" / "ix"), bad)
    assert not os.path.exists(str(tmp_path / "w"))


def test_cli_refuses_a_query_file_with_a_nan(tmp_path):
    """bin/bang_search on a query file that holds a NaN: non-zero exit, the message, no row of the result table."""
    import re
    import bang_amd
    from bang_amd import formats
    ix, q = FR.get("d68", "unscaled")
    Q = q.shape[0]
    prefix = str(tmp_path / "ix")
    formats.write_index(prefix, ix)
    bad = q.copy()
    bad[Q // 2, ix.D - 1] = np.nan
    formats.write_bin(prefix + "_query.bin", bad)
    ids, d, _ = _exact("d68", "unscaled", 37)
    formats.write_truthset(prefix + "_gt.bin", ids.astype(np.uint32), np.ascontiguousarray(d.T))
    exe = os.path.join(os.path.dirname(os.path.dirname(bang_amd.lib_path())), "bin", "bang_search")
    r = subprocess.run([exe, prefix, prefix + "_query.bin", prefix + "_gt.bin", str(Q), str(K), "float", "l2", "auto"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0, (r.stdout[-1000:], r.stderr[-1000:])
    assert "GPUassert: bang_query" in r.stderr and f"query {Q // 2}, dimension {ix.D - 1} " in r.stderr, r.stderr[-1000:]
    assert not [ln for ln in r.stdout.splitlines() if re.match(r"^\d+\t", ln)], r.stdout[-1000:]
