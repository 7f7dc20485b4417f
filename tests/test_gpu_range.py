"""Range search (option range_hits, Engine.set_radii, bang_k_search_exact_range: search_exact_range_kernel and search_exact_range_pull_kernel of
csrc/bang_search_exact.hip; bang_k_range_sort: range_sort_kernel of csrc/bang_range.hip) on a GPU, against the CPU reference of
tests/range_reference.py: hit ids, distance bits, order, counts and offered of every query, and -- the walk is untouched -- top-k, the four per-query
counters and the candidate log of the same engine run without radii.  32 queries per fixture; worklists of 10, 37 and 152; every radius of
tests/range_inputs.py at a capacity of 512, rank400 at 64 as well; graph entries in HBM and pulled rows.  Then int8, the toy inputs and the 65-id
seed list in every layout, an exclusion set on top, one wave per workgroup, two lanes, one allocation queried three times, device buffers,
range_hits without radii, the sort kernel alone on crafted rows, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import beam_inputs as BI
import edge_inputs as E
import exclude_reference as X
import range_inputs as RI
import range_reference as RR

pytestmark = pytest.mark.gpu

K = 10
NQ = 32
LS = (10, 37, 152)
CAP = 512
FORMS = {"hbm": dict(graph=1, distance=1), "pull": dict(graph=0, pull=1, distance=1)}
ERR_ARG = -1
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _ref(name, ix):
    return _cached(("ref", name), lambda: RR.Reference(ix))


def _traces(name, ix, q, L):
    return _cached((name, q.shape, L), lambda: _ref(name, ix).evaluated_all(q, L))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(e, q, k, L, radii=None, cap=CAP, Qcap=None):
    """A loaded, unallocated engine: one batch with the radii or without.  -> dict"""
    Q = q.shape[0]
    e.set_option("range_hits", cap)
    e.set_searchparams(k, L)
    e.alloc(Q if Qcap is None else Qcap)
    if radii is not None:
        e.set_radii(radii)
    e.init(Q)
    ids, d = e.query(q)
    log, log_n = e.candidate_log(Q, L)
    out = dict(ids=ids, d=d, counters=e.query_counters(Q), log=log, log_n=log_n, stats=e.stats())
    if radii is not None:
        out["counts"], out["offered"] = e.range_counts(Q)
        out["lims"], out["hit_ids"], out["hit_d"] = e.range_results(Q)
    e.free()
    return out


def _check_range(got, want, cap, what):
    """want = RR.collect_all(...)"""
    lims, ids, d, counts, offered = want
    assert np.array_equal(got["offered"], offered), what
    assert np.array_equal(got["counts"], counts), what
    assert np.array_equal(got["lims"], lims) and got["lims"][0] == 0, what
    assert got["hit_ids"].dtype == np.uint64 and np.array_equal(got["hit_ids"], ids), what
    assert np.array_equal(_bits(got["hit_d"]), _bits(d)), what
    s = got["stats"]
    assert s["range_launches"] == 1 and s["front_launches"] == 1 and s["range_hits"] == cap and s["range_queries"] == len(counts), (what, s)
    assert s["range_truncated"] == int((offered > cap).sum()) and s["label_launches"] == 0, (what, s)


def _check_walk(got, base, what):
    """The same engine's run without radii: top-k ids and distance bits, the four counters, the candidate log."""
    assert np.array_equal(got["ids"], base["ids"]) and np.array_equal(_bits(got["d"]), _bits(base["d"])), what
    assert np.array_equal(got["counters"], base["counters"]) and np.array_equal(got["log_n"], base["log_n"]), what
    for i in range(len(got["log_n"])):
        assert np.array_equal(got["log"][i, :got["log_n"][i]], base["log"][i, :base["log_n"][i]]), (what, i)


def _check_base(base, traces, k, what):
    for i, t in enumerate(traces):
        n = min(k, len(t.wl_ids))
        assert np.array_equal(base["ids"][i, :n], t.wl_ids[:n].astype(np.uint64)) and (base["ids"][i, n:] == RR.PAD_ID).all(), (what, i)
        assert np.array_equal(_bits(base["d"][:n, i]), _bits(t.wl_dists[:n])), (what, i)
        assert tuple(base["counters"][i]) == tuple(t.stats), (what, i)
        assert np.array_equal(base["log"][i, :base["log_n"][i]], t.log), (what, i)


def _case(name, ix, q, opts, Ls, cases, excluded=None):
    """cases(ix, q) -> [(label, radii f32 [Q], cap)]"""
    import bang_amd
    with bang_amd.Engine(ix.dtype, **opts) as e:
        e.load_index(ix)
        if excluded is not None:
            e.set_excluded(excluded)
        for L in Ls:
            tr = _traces(name, ix, q, L)
            base = _run(e, q, K, L)                                       # range_hits set, no radii: today's launches
            s = base["stats"]
            assert s["range_launches"] == 0 and s["range_queries"] == 0 and s["range_truncated"] == 0 and s["front_launches"] == 1, s
            if excluded is None:
                _check_base(base, tr, K, (name, L, "no radii"))
            else:
                assert s["exclude_launches"] == 1, s
            for label, radii, cap in cases(ix, q):
                got = _run(e, q, K, L, radii, cap)
                _check_range(got, RR.collect_all(tr, radii, cap, excluded), cap, (name, L, label, cap))
                _check_walk(got, base, (name, L, label, cap))
                assert got["stats"]["exclude_launches"] == (0 if excluded is None else 1)
        e.unload()


def _named_cases(name, names=RI.NAMES):
    def make(ix, q):
        ref = _ref(name, ix)
        out = [(n, RI.radii(n, ref, ix, q), CAP) for n in names]
        if "rank400" in names:
            out.append(("rank400", RI.radii("rank400", ref, ix, q), 64))
        return out
    return make


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_range_walks(request, fixture, form, L):
    ix, q, _, _ = request.getfixturevalue(fixture)
    _case(fixture, ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (L,), _named_cases(fixture))


@pytest.mark.parametrize("form", list(FORMS))
def test_int8(small_i8, form):
    ix, q, _, _ = small_i8
    _case("small_i8", ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (24,), _named_cases("small_i8"))


def _toy_cases(levels_of):
    """+inf, -1, and the squared distance of a chosen level difference per dimension (the toy vectors are constant per node)"""
    def make(ix, q):
        Q = q.shape[0]
        out = [("all", np.full(Q, np.inf, np.float32), CAP), ("none", np.full(Q, -1.0, np.float32), CAP), ("all/1", np.full(Q, np.inf, np.float32), 1),
               ("all/2", np.full(Q, np.inf, np.float32), 2)]
        for lv in levels_of:
            out.append((f"level{lv}", np.full(Q, float(lv * lv * ix.D), np.float32), CAP))
        return out
    return make


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype,D", E.TOY_LAYOUTS)
def test_toy_inputs(dtype, D, form):
    """The chain (a hit in the cap iteration, the nearest node the walk ever evaluates and never merges), the short worklist, the row that lists
    node 2 twice (offered > count), the distance ties of the toy graphs."""
    ix, q = E.chain(dtype, D)
    for L in (10, 152):
        last = 255 - (L + 49)                                                # the level of the cap iteration's survivor; the query sits at level 0
        assert RR.Reference(ix).evaluated(q[0], L).iters[-1][0] == L + 49
        _case(("chain", dtype, D), ix, q, FORMS[form], (L,), _toy_cases((last, last + 1, 254)))
    ix, q = BI.row_dup(dtype, D)
    t = RR.Reference(ix).evaluated(q[0], 10)
    assert RR.collect(t, np.inf, CAP)[2] > RR.collect(t, np.inf, CAP)[3]
    _case(("row_dup", dtype, D), ix, q, FORMS[form], (10,), _toy_cases((20, 30)))
    ix, q = E.short_worklist(dtype, D)
    _case(("short_worklist", dtype, D), ix, q, FORMS[form], (10,), _toy_cases((10, 20)))
    ix, q = E.toy_named("tie", dtype, D)
    _case(("tie", dtype, D), ix, q, FORMS[form], (10,), _toy_cases((20,)))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype,D", E.SEED65_LAYOUTS)
@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_seed65(variant, dtype, D, form):
    """65 survivors in the seed iteration: all 65 within the radius (node 64, the one no lane holds, behind the first 64), node 64 alone or with its
    ties, and capacities that cut the log at and around slot 64."""
    ix, q = E.seed65(dtype, variant, D)
    t = RR.Reference(ix).evaluated(q[0], 10)
    d64 = float(t.iters[0][2][64])
    assert len(t.iters[0][1]) == 65 and int(t.iters[0][1][64]) == E.SEED65_LAST

    def cases(ix_, q_):
        Q = q_.shape[0]
        inf = np.full(Q, np.inf, np.float32)
        return [("all", inf, CAP), ("all/64", inf, 64), ("all/65", inf, 65), ("all/63", inf, 63), ("node64", np.full(Q, d64, np.float32), CAP),
                ("node64/1", np.full(Q, d64, np.float32), 1), ("none", np.full(Q, np.nan, np.float32), CAP)]
    _case(("seed65", dtype, variant, D), ix, q, FORMS[form], (10,), cases)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("fixture", ("small_u8", "small_f32"))
def test_tie_heavy(request, fixture, form):
    """Most of a query's hits tie: equal distance bits come out ordered by id."""
    ix, q = E.tie_heavy(*request.getfixturevalue(fixture)[:2], n_queries=8)
    name = ("tie_heavy", fixture)
    want = RR.collect_all(_traces(name, ix, q, 37), np.full(8, np.inf, np.float32), 4096)
    same = _bits(want[2])[1:] == _bits(want[2])[:-1]
    assert same.any()
    _case(name, ix, q, FORMS[form], (37,), lambda ix_, q_: [("all", np.full(8, np.inf, np.float32), 4096), ("all/100", np.full(8, np.inf, np.float32), 100),
                                                            ("two", np.full(8, 2.0, np.float32), CAP)])


@pytest.mark.parametrize("mask", ("rand30", "edges"))
@pytest.mark.parametrize("form", list(FORMS))
def test_with_an_exclusion_set(small_u8, form, mask):
    """A node of the engine's exclusion set is no hit; the top-k goes through bang_k_worklist_pick as before."""
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    excluded = X.make_mask(mask, ix)
    tr = _traces("small_u8", ix, q, 37)
    r = RI.radii("rank100", _ref("small_u8", ix), ix, q)
    with_x, without = RR.collect_all(tr, r, CAP, excluded), RR.collect_all(tr, r, CAP)
    if mask == "rand30":
        assert (with_x[3] < without[3]).any()
    _case("small_u8", ix, q, FORMS[form], (37,), _named_cases("small_u8", ("rank100", "all", "mixed")), excluded=excluded)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_wave_per_workgroup(small_u8, monkeypatch, form):
    """One workgroup of one wave runs every query in turn (the wave cap alone repeats the default launch: 32 queries are 32 one-wave workgroups
    already).  Full workgroups: tests/test_gpu_launch_shapes.py."""
    ix, q, _, _ = small_u8
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    _case("small_u8", ix, np.ascontiguousarray(q[:NQ]), FORMS[form], (37,), _named_cases("small_u8", ("rank100", "rank400", "mixed")))


@pytest.mark.parametrize("form", list(FORMS))
def test_two_lanes(small_u8, form):
    ix, q, _, _ = small_u8
    _case("small_u8", ix, np.ascontiguousarray(q[:NQ]), dict(FORMS[form], lanes=2), (37,), _named_cases("small_u8", ("rank100", "rank400", "mixed")))


@pytest.mark.parametrize("form", list(FORMS))
def test_one_allocation_three_queries(small_u8, form):
    """Radii set, replaced (a smaller batch in a larger allocation), cleared on one allocation: the last run is today's run."""
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    L = 37
    tr = _traces("small_u8", ix, q, L)
    ref = _ref("small_u8", ix)
    with bang_amd.Engine(ix.dtype, range_hits=CAP, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_searchparams(K, L)
        e.alloc(NQ + 5)
        for name in ("rank400", "rank5"):
            r = RI.radii(name, ref, ix, q)
            e.set_radii(r)
            e.init(NQ)
            e.query(q)
            got = dict(stats=e.stats())
            got["counts"], got["offered"] = e.range_counts(NQ)
            got["lims"], got["hit_ids"], got["hit_d"] = e.range_results(NQ)
            _check_range(got, RR.collect_all(tr, r, CAP), CAP, name)
            counts7, offered7 = e.range_counts(7)                                # (the first queries of the batch)
            assert np.array_equal(counts7, got["counts"][:7]) and np.array_equal(offered7, got["offered"][:7])
        e.set_radii(2.0, Q=7)                                                    # a scalar is broadcast
        e.init(NQ)
        with pytest.raises(bang_amd.BangError, match="radii"):                   # a batch of another size than the radii's
            e.query(q)
        e.init(7)
        e.query(q[:7])
        got = e.range_results(7)
        want = RR.collect_all(tr[:7], np.full(7, 2.0, np.float32), CAP)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
        e.clear_radii()
        e.init(NQ)
        ids, d = e.query(q)
        log, log_n = e.candidate_log(NQ, L)
        _check_base(dict(ids=ids, d=d, counters=e.query_counters(NQ), log=log, log_n=log_n), tr, K, "cleared")
        s = e.stats()
        assert s["range_launches"] == 0 and s["range_queries"] == 0 and s["range_truncated"] == 0 and s["range_hits"] == CAP
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.range_counts(NQ)
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.range_results(NQ)
        e.free()
        e.unload()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("with_dists", (True, False))
def test_results_into_device_buffers(small_u8, with_dists, form):
    """bang_query_dev_e: the k results stay in the caller's device buffers, the range answer is fetched as ever."""
    import torch
    import bang_amd
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    L = 37
    tr = _traces("small_u8", ix, q, L)
    r = RI.radii("rank100", _ref("small_u8", ix), ix, q)
    d_ids = torch.zeros((NQ, K), dtype=torch.int64, device="cuda")
    d_d = torch.zeros((K, NQ), dtype=torch.float32, device="cuda")
    with bang_amd.Engine(ix.dtype, range_hits=CAP, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_searchparams(K, L)
        e.alloc(NQ)
        e.set_radii(r)
        e.init(NQ)
        e.query_dev(q, d_ids.data_ptr(), d_d.data_ptr() if with_dists else 0)
        torch.cuda.synchronize()
        ids = d_ids.cpu().numpy().view(np.uint64)
        for i, t in enumerate(tr):
            assert np.array_equal(ids[i], t.wl_ids[:K].astype(np.uint64)), i
            if with_dists:
                assert np.array_equal(d_d[:, i].cpu().numpy().view(np.uint32), _bits(t.wl_dists[:K])), i
        if not with_dists:
            assert not d_d.cpu().numpy().any()
        got = dict(stats=e.stats())
        got["counts"], got["offered"] = e.range_counts(NQ)
        got["lims"], got["hit_ids"], got["hit_d"] = e.range_results(NQ)
        _check_range(got, RR.collect_all(tr, r, CAP), CAP, "dev")
        e.free()
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the sort kernel alone
# ---------------------------------------------------------------------------------------------------------------------
def _sort_rows(cap, rows, q0=0, nq=None):
    """rows: [(ids u32 [n <= cap], dists f32 [n], offered)] -> the buffers after bang_k_range_sort on rows q0 .. q0 + nq - 1"""
    from bang_amd import binding as B
    Q = len(rows)
    nq = Q - q0 if nq is None else nq
    ids = np.full((Q, cap), 0xDEADBEEF, np.uint32)
    d = np.full((Q, cap), -7.0, np.float32)
    off = np.zeros(Q, np.uint32)
    for i, (a, b, o) in enumerate(rows):
        ids[i, :len(a)] = a
        d[i, :len(b)] = b
        off[i] = o
    cnt = np.full(Q, 0xFFFFFFFF, np.uint32)
    bufs = [B.DeviceBuffer.from_numpy(x) for x in (ids, d, off, cnt)]
    try:
        f = B.lib().bang_k_range_sort
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        assert f(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, cap, q0, nq, Q, bufs[3].ptr, None) == 0, B.lib().bang_last_error()
        B.sync()
        return (bufs[0].download(np.uint32, (Q, cap)), bufs[1].download(np.float32, (Q, cap)), bufs[3].download(np.uint32, (Q,)), ids, d)
    finally:
        for b in bufs:
            b.free()


def _check_sorted(cap, rows, q0=0, nq=None):
    out_ids, out_d, cnt, in_ids, in_d = _sort_rows(cap, rows, q0, nq)
    nq = len(rows) - q0 if nq is None else nq
    for i, (a, b, o) in enumerate(rows):
        if not q0 <= i < q0 + nq:                                               # not this launch's row: untouched
            assert np.array_equal(out_ids[i], in_ids[i]) and np.array_equal(_bits(out_d[i]), _bits(in_d[i])) and cnt[i] == 0xFFFFFFFF, i
            continue
        n = min(int(o), cap)
        want = np.unique(RR.keys(in_ids[i, :n], in_d[i, :n]))
        assert cnt[i] == len(want), (i, cnt[i], len(want))
        assert np.array_equal(RR.keys(out_ids[i, :cnt[i]], out_d[i, :cnt[i]]), want), i


def _crafted(cap, rng):
    def row(n, offered=None, ids=None, d=None):
        ids = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if ids is None else np.asarray(ids, np.uint32)
        d = rng.integers(0, 50, n).astype(np.float32) if d is None else np.asarray(d, np.float32)
        return ids, d, n if offered is None else offered
    rows = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096):
        if n <= cap:
            rows.append(row(n))
    n = min(cap, 300)
    rows.append(row(n, ids=np.full(n, 9), d=np.full(n, 3.0)))                             # all-equal keys
    if n > 10:                                                                             # duplicates at both ends
        rows.append(row(n, ids=np.r_[np.zeros(5), np.arange(n - 10), np.full(5, n)], d=np.r_[np.zeros(5), np.ones(n - 10), np.full(5, 2.0)]))
    rows.append(row(cap, offered=cap + 1))                                                 # offered > cap
    rows.append(row(cap, offered=0xFFFFFFFF))
    rows.append(row(min(cap, 70), d=np.zeros(min(cap, 70))))                               # distance 0: the id orders
    rows.append(row(min(cap, 200), ids=np.full(min(cap, 200), 0xFFFFFFFF), d=np.full(min(cap, 200), np.float32(3.402823e38))))   # the largest key a hit can have
    rows.append(row(min(cap, 64), ids=np.arange(min(cap, 64))[::-1], d=np.arange(min(cap, 64))[::-1]))                          # descending input
    return rows


@pytest.mark.parametrize("cap", (4096, 512, 100, 64, 1))
def test_range_sort_against_numpy(cap):
    rng = np.random.default_rng(cap)
    rows = _crafted(cap, rng)
    _check_sorted(cap, rows)
    _check_sorted(cap, rows, q0=3, nq=len(rows) - 5)                                       # a lane's slice of the batch


# ---------------------------------------------------------------------------------------------------------------------
# call order and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_call_order_and_capacity(small_u8):
    import bang_amd
    from bang_amd import binding as B
    ix, q, _, _ = small_u8
    q = np.ascontiguousarray(q[:NQ])
    r = np.full(NQ, np.inf, np.float32)
    with bang_amd.Engine(ix.dtype, graph=1, distance=1) as e:
        e.load_index(ix)
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):            # radii live in an allocation
            e.set_radii(r)
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        with pytest.raises(bang_amd.BangError, match="range_hits"):            # range search is off
            e.set_radii(r)
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):            # the rule of the options consumed by bang_alloc
            e.set_option("range_hits", 64)
        e.free()
        e.set_option("range_hits", 64)
        e.alloc(NQ)
        with pytest.raises(bang_amd.BangError, match="exceed"):
            e.set_radii(np.zeros(NQ + 1, np.float32))
        e.set_radii(r)
        e.init(NQ)
        e.query(q)
        counts, offered = e.range_counts(NQ)
        with pytest.raises(bang_amd.BangError, match="asked for"):
            e.range_counts(NQ + 1)
        total = int(counts.sum())
        assert total > 0 and (offered > 64).all() and e.stats()["range_truncated"] == NQ
        # a capacity below lims[nq]: BANG_ERR_ARG, nothing written
        fn = B.lib().bang_get_range_results
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        lims = np.full(NQ + 1, 77, np.uint64)
        ids = np.full(total, 77, np.uint64)
        d = np.full(total, 77, np.float32)
        assert fn(e._h, lims.ctypes.data, ids.ctypes.data, d.ctypes.data, total - 1) == ERR_ARG
        assert "capacity" in B.lib().bang_last_error().decode()
        assert (lims == 77).all() and (ids == 77).all() and (d == 77).all()
        assert fn(e._h, lims.ctypes.data, ids.ctypes.data, d.ctypes.data, total) == 0 and lims[0] == 0 and lims[NQ] == total
        e.free()
        e.alloc(NQ)                                                            # a new allocation has no batch to report on
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.range_counts(NQ)
        assert e.stats()["range_launches"] == 0 and e.stats()["range_truncated"] == 0
        e.free()
        e.unload()


def test_radii_and_label_filters_do_not_combine(small_u8):
    """Refused at whichever of the two setters comes second."""
    import bang_amd
    ix, q, _, _ = small_u8
    r = np.full(NQ, 1.0, np.float32)
    w = np.ones(NQ, np.uint32)
    with bang_amd.Engine(ix.dtype, graph=1, distance=1, range_hits=64) as e:
        e.load_index(ix)
        e.set_labels(np.ones(ix.N, np.uint32))
        e.set_searchparams(K, 37)
        e.alloc(NQ)
        e.set_filters(w, w)
        with pytest.raises(bang_amd.BangError, match="filters"):
            e.set_radii(r)
        e.clear_filters()
        e.set_radii(r)
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.set_filters(w, w)
        e.clear_radii()
        e.set_filters(w, w)
        e.free()
        e.unload()


@pytest.mark.parametrize("opts,fixture", ((dict(graph=1), "small_u8"), (dict(graph=1, distance=1, beam=2), "small_u8"),
                                          (dict(graph=0, pull=1, distance=1, vectors_fp16=1), "small_f32"), (dict(graph=1, distance=1), "u8_48")),
                         ids=("pq_walk", "beam", "fp16", "wide"))
def test_forms_without_a_range_kernel_are_refused(request, opts, fixture):
    """Refused at bang_alloc with `range` in the message; the same engine runs its batch with range_hits = 0."""
    import bang_amd
    if fixture == "u8_48":
        import highdim_inputs as H
        ix, q = H.get("u8_48")
    else:
        ix, q, _, _ = request.getfixturevalue(fixture)
    q = np.ascontiguousarray(q[:8])
    with bang_amd.Engine(ix.dtype, range_hits=64, **opts) as e:
        e.load_index(ix)
        e.set_searchparams(K, 24)
        with pytest.raises(bang_amd.BangError, match="range"):
            e.alloc(8)
        e.set_option("range_hits", 0)
        e.alloc(8)
        e.init(8)
        ids, _ = e.query(q)
        assert (ids != RR.PAD_ID).any() and e.stats()["range_launches"] == 0
        e.free()
        e.unload()
