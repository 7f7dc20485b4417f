"""Adjacency rows in the padding of the PQ code table (option "rows_pad", pull mode) on the GPU: only WHERE a row is read from changes.

The index is tests/rows_pad_inputs.py's (N = 1003, m = 70: n_pad = 200; with BANG_ROWS_HBM_MAX_ROWS = 256 the HBM copy holds [200, 456) and the rest is
pulled).  Every run is compared with the oracle (ids, distance bits, per-query iterations / candidates / evaluations / ids fetched), with the run
without padded rows, and its candidate log with the CPU walk of tests/wordfilter_reference.py.

Addresses above 4 GiB: the padded branch of the search kernel is compiled for lines of 128 bytes (the stride is a constant of the instance), so the
stretched-stride hook of tests/test_gpu_offsets64.py does not reach it -- a padded row's offset passes 2^32 at row 6 710 887 only.  The 64-bit
arithmetic is checked on the CPU (tests/test_rows_pad_layout.py: row 2^23, row 6 710 887, the last row of 10^9 nodes, and the kernel's split into a
uniform row part and a lane part)."""
import ctypes as C

import numpy as np
import pytest

import rows_pad_inputs as I

pytestmark = pytest.mark.gpu
GRAPH_HOST = 0


@pytest.fixture(scope="module")
def logs():
    """the CPU walk's candidate logs of the 64 queries (it is the oracle's walk: its per-query counters are compared below)"""
    from wordfilter_reference import Reference
    ix, q = I.index()
    ref = Reference(ix)
    out, st = [], []
    for i in range(I.Q):
        log = []
        st.append(ref.search_one(q[i], I.K, I.L, "split", log=log)[2])
        out.append(np.array(log, np.uint32))
    assert np.array_equal(np.array(st), I.reference(I.Q)[2])
    return out


def run(nq, monkeypatch, rows_pad, max_rows=None, env=(), spare=None, rows_hbm=64, after_load=None, **opts):
    """One engine: load, [after_load(engine)], alloc, query.  max_rows / spare: the test hooks BANG_ROWS_HBM_MAX_ROWS (cap on the copy) and
    BANG_ROWS_HBM_SPARE_ROWS (rows the spare HBM counts as holding: below N, "the rows do not all fit" and both autos turn on)."""
    import bang_amd
    ix, q = I.index()
    for k in ("BANG_SPEC_ROWS", "BANG_SUMM_ITERS", "BANG_ROWS_PAD", "BANG_ROWS_HBM_MAX_ROWS", "BANG_ROWS_HBM_SPARE_ROWS"):
        monkeypatch.delenv(k, raising=False)
    if max_rows is not None:
        monkeypatch.setenv("BANG_ROWS_HBM_MAX_ROWS", str(max_rows))
    if spare is not None:
        monkeypatch.setenv("BANG_ROWS_HBM_SPARE_ROWS", str(spare))
    for k, v in env:
        monkeypatch.setenv(k, v)
    if rows_pad is not None:
        opts["rows_pad"] = rows_pad
    with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1, rows_hbm=rows_hbm, **opts) as e:
        e.load_index(ix)
        n_pad = e.rows_pad()
        if after_load:
            after_load(e)
        e.set_searchparams(I.K, I.L)
        e.alloc(nq)
        e.init(nq)
        ids, dists = e.query(q[:nq])
        out = dict(ids=ids, dists=dists, counters=e.query_counters(nq), stats=e.stats(), n_pad=n_pad, n_pad_after=e.rows_pad(), codes=e.codes(0, ix.N))
        out["log"], out["cnt"] = e.candidate_log(nq, I.L)
        e.free()
        e.unload()
    return out


def same_answers(got, nq):
    ids_o, dists_o, st_o = I.reference(nq)
    assert np.array_equal(got["ids"], ids_o) and np.array_equal(got["dists"].view(np.uint32), dists_o.view(np.uint32))
    assert np.array_equal(got["counters"], st_o)


def same_log(a, b):
    """the candidate logs agree: the counts, and every query's entries up to its count (what lies behind is not written)"""
    return bool(np.array_equal(a["cnt"], b["cnt"]) and all(np.array_equal(a["log"][i, :n], b["log"][i, :n]) for i, n in enumerate(a["cnt"])))


def expanded(got, nq):
    """ids of the rows the batch read: every log entry but the medoid's (the seed list is on the device)"""
    return np.concatenate([got["log"][i, 1:got["cnt"][i]] for i in range(nq)])


def check_sources(got, nq, n_pad, n_copy):
    """rows_from_own_hbm + pulled rows = expanded rows, each share what the candidate log says"""
    s, ex = got["stats"], expanded(got, nq)
    assert s["graph_pull"] == 1 and s["rows_in_hbm"] == n_pad + n_copy and s["rows_from_peer"] == 0
    assert len(ex) == s["candidates"] - nq
    in_pad, in_copy = int((ex < n_pad).sum()), int(((ex >= n_pad) & (ex < n_pad + n_copy)).sum())
    assert s["rows_from_own_hbm"] == in_pad + in_copy and s["pulled_bytes"] == 256 * (len(ex) - in_pad - in_copy)
    return in_pad, in_copy, len(ex) - in_pad - in_copy


@pytest.fixture(scope="module")
def plain():
    """the run without padded rows, copy [0, 256): what every other run must equal"""
    mp = pytest.MonkeyPatch()
    try:
        got = run(I.Q, mp, 0, I.N_COPY)
    finally:
        mp.undo()
    same_answers(got, I.Q)
    assert got["n_pad"] == 0
    return got


def test_three_sources_same_bits_and_every_seam_walked(libbang, monkeypatch, plain, logs):
    ix, _ = I.index()
    got = run(I.Q, monkeypatch, 1, I.N_COPY)
    assert got["n_pad"] == got["n_pad_after"] == I.N_PAD == ix.N // 5
    same_answers(got, I.Q)
    for k in ("ids", "counters"):
        assert np.array_equal(got[k], plain[k]), k
    assert same_log(got, plain)
    assert np.array_equal(got["dists"].view(np.uint32), plain["dists"].view(np.uint32))
    for k in ("iterations", "dist_evals", "fetched", "candidates", "filter_loads_skipped"):
        assert got["stats"][k] == plain["stats"][k], k
    assert np.array_equal(got["codes"], ix.codes) and np.array_equal(plain["codes"], ix.codes)       # the fill left every code byte alone
    for i in range(I.Q):
        assert np.array_equal(got["log"][i, :got["cnt"][i]], logs[i]), i
    # all three sources were read, and the parents on both sides of both seams were expanded; so were rows of 1, 13, 14, 15 and 64 ids
    in_pad, in_copy, pulled = check_sources(got, I.Q, I.N_PAD, I.N_COPY)
    assert in_pad > 0 and in_copy > 0 and pulled > 0
    ex = set(int(x) for x in expanded(got, I.Q))
    assert set(I.SEAMS) <= ex
    deg = ix.degrees()
    assert {int(deg[s]) for s in I.SEAMS} == {1, 13, 14, 15} and any(deg[p] == 64 for p in ex)
    assert I.N_PAD - 1 in ex and I.N_PAD in ex and I.N_PAD + I.N_COPY - 1 in ex and I.N_PAD + I.N_COPY in ex
    # ... and without them the same rows came from the copy [0, 256) and over PCIe
    check_sources(plain, I.Q, 0, I.N_COPY)


def test_padded_rows_without_a_copy(libbang, monkeypatch, plain):
    got = run(I.Q, monkeypatch, 1, 0)
    assert got["n_pad"] == I.N_PAD
    same_answers(got, I.Q)
    assert same_log(got, plain)
    in_pad, in_copy, pulled = check_sources(got, I.Q, I.N_PAD, 0)
    assert in_pad > 0 and in_copy == 0 and pulled > 0


@pytest.mark.parametrize("env", [(("BANG_SPEC_ROWS", "1"),), (("BANG_SPEC_ROWS", "2"),), (("BANG_SUMM_ITERS", "-1"),), (("BANG_SUMM_ITERS", "1"),),
                                 (("BANG_SPEC_ROWS", "2"), ("BANG_SUMM_ITERS", "-1"))], ids=lambda e: "+".join(f"{k[5:]}={v}" for k, v in e))
def test_both_row_request_forms_and_both_summary_settings(libbang, monkeypatch, plain, env):
    got = run(I.Q, monkeypatch, 1, I.N_COPY, env=env)
    assert got["n_pad"] == I.N_PAD
    same_answers(got, I.Q)
    assert same_log(got, plain)
    check_sources(got, I.Q, I.N_PAD, I.N_COPY)


@pytest.mark.parametrize("nq", [1, 700])
def test_one_query_and_more_queries_than_waves(libbang, monkeypatch, nq):
    got = run(nq, monkeypatch, 1, I.N_COPY)
    assert got["n_pad"] == I.N_PAD
    same_answers(got, nq)
    in_pad, _, _ = check_sources(got, nq, I.N_PAD, I.N_COPY)
    assert in_pad > 0


def test_word_filter_kernel_reads_them_too(libbang, monkeypatch):
    """filter_layout = 1 runs the same hand-over (search_wf_kernel): same answers with and without padded rows"""
    a = run(I.Q, monkeypatch, 0, I.N_COPY, filter_layout=1)
    b = run(I.Q, monkeypatch, 1, I.N_COPY, filter_layout=1)
    assert b["n_pad"] == I.N_PAD and b["stats"]["filter_layout"] == 1
    for k in ("ids", "counters"):
        assert np.array_equal(a[k], b[k]), k
    assert same_log(a, b)
    assert np.array_equal(a["dists"].view(np.uint32), b["dists"].view(np.uint32))
    check_sources(b, I.Q, I.N_PAD, I.N_COPY)


def test_auto_leaves_an_index_that_fits_hbm_alone(libbang, monkeypatch, plain):
    got = run(I.Q, monkeypatch, -1, I.N_COPY)
    assert got["n_pad"] == 0
    assert same_log(got, plain)
    check_sources(got, I.Q, 0, I.N_COPY)


SPARE = 500          # of N = 1003 rows: the rows do not all fit -> auto fills the padding (200 rows) and the copy takes the next 500


def same_run(a, b):
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["dists"].view(np.uint32), b["dists"].view(np.uint32))
    assert np.array_equal(a["counters"], b["counters"]) and same_log(a, b)


def test_auto_turns_on_where_the_rows_do_not_all_fit(libbang, monkeypatch, plain):
    """both options on auto, as in production: padded rows [0, 200), the copy the 500 rows behind them"""
    got = run(I.Q, monkeypatch, None, spare=SPARE, rows_hbm=-1)
    assert got["n_pad"] == got["n_pad_after"] == I.N_PAD
    same_answers(got, I.Q)
    same_run(got, plain)
    in_pad, in_copy, pulled = check_sources(got, I.Q, I.N_PAD, SPARE)
    assert in_pad > 0 and in_copy > 0 and pulled > 0
    off = run(I.Q, monkeypatch, 0, spare=SPARE, rows_hbm=-1)            # the same load without the option: the parent's copy [0, 500)
    assert off["n_pad"] == 0
    same_run(off, plain)
    check_sources(off, I.Q, 0, SPARE)


@pytest.mark.parametrize("spare", [803, 900, 1002])
def test_auto_copy_is_kept_where_the_spare_hbm_holds_most_rows(libbang, monkeypatch, plain, spare):
    """0.8 N <= spare < N: the padded rows take 200, the copy takes ALL the others (803 <= spare) -- not none of them"""
    got = run(I.Q, monkeypatch, None, spare=spare, rows_hbm=-1)
    assert got["n_pad"] == I.N_PAD
    same_run(got, plain)
    in_pad, in_copy, pulled = check_sources(got, I.Q, I.N_PAD, I.N - I.N_PAD)
    assert in_pad > 0 and in_copy > 0 and pulled == 0
    off = run(I.Q, monkeypatch, 0, spare=spare, rows_hbm=-1)
    check_sources(off, I.Q, 0, spare)


def test_auto_off_where_the_rows_fit(libbang, monkeypatch, plain):
    got = run(I.Q, monkeypatch, None, spare=I.N, rows_hbm=-1)             # spare HBM holds every row: neither the padding nor a copy (the caller chose the host)
    assert got["n_pad"] == 0
    same_run(got, plain)
    check_sources(got, I.Q, 0, 0)


@pytest.mark.parametrize("opts", [dict(distance=1), dict(walker=1), dict(persistent=0)], ids=lambda o: "+".join(f"{k}={v}" for k, v in o.items()))
def test_auto_gives_the_padded_rows_up_for_a_form_that_cannot_read_them(libbang, monkeypatch, opts):
    """filled at load, given up at bang_alloc: no padded rows, the copy starts over at row 0, and the run is the run of rows_pad = 0"""
    got = run(I.Q, monkeypatch, None, spare=SPARE, rows_hbm=-1, **opts)
    off = run(I.Q, monkeypatch, 0, spare=SPARE, rows_hbm=-1, **opts)
    assert got["n_pad"] == I.N_PAD and got["n_pad_after"] == 0 and off["n_pad"] == 0
    same_run(got, off)
    for k in ("graph_pull", "rows_in_hbm", "rows_from_own_hbm", "pulled_bytes", "candidates", "walker_rows", "search_kernel"):
        assert got["stats"][k] == off["stats"][k], k
    if "distance" in opts:
        from exact_reference import Reference
        ix, q = I.index()
        ids_o, dists_o, st_o = Reference(ix).search(q[:I.Q], I.K, I.L, "exact")[:3]
        assert np.array_equal(got["ids"], ids_o) and np.array_equal(got["dists"].view(np.uint32), dists_o.view(np.uint32)) and np.array_equal(got["counters"], st_o)
        in_pad, in_copy, pulled = check_sources(got, I.Q, 0, SPARE)
        assert in_copy > 0 and pulled > 0
    else:                                                   # the PQ walk in another form: the oracle's results (the per-iteration loop reports no iteration counts)
        ids_o, dists_o, _ = I.reference(I.Q)
        assert np.array_equal(got["ids"], ids_o) and np.array_equal(got["dists"].view(np.uint32), dists_o.view(np.uint32))


def test_auto_gives_the_padded_rows_up_for_peer_rows(libbang, monkeypatch, plain):
    seen = {}

    def slice_(e):
        assert e.rows_capacity() > 0 and e.rows_pad() == I.N_PAD          # the query alone changes nothing
        e.rows_slice(0, 300)
        seen["after_slice"] = e.rows_pad()
    got = run(I.Q, monkeypatch, None, spare=SPARE, rows_hbm=-1, after_load=slice_)
    assert got["n_pad"] == I.N_PAD and seen["after_slice"] == 0 and got["n_pad_after"] == 0
    same_run(got, plain)
    check_sources(got, I.Q, 0, 300)

    def export(e):
        _, first, rows = e.rows_export()
        seen["export"] = (first, rows, e.rows_pad())
    got = run(I.Q, monkeypatch, None, spare=SPARE, rows_hbm=-1, after_load=export)
    assert seen["export"] == (0, SPARE, 0)                                # the copy was started over at row 0 before its handle went out
    same_run(got, plain)
    check_sources(got, I.Q, 0, SPARE)


def test_unload_resets_and_a_reload_decides_anew(libbang, monkeypatch, plain):
    import bang_amd
    ix, q = I.index()
    monkeypatch.setenv("BANG_ROWS_HBM_SPARE_ROWS", str(SPARE))
    monkeypatch.delenv("BANG_ROWS_HBM_MAX_ROWS", raising=False)

    def search(e):
        e.set_searchparams(I.K, I.L)
        e.alloc(I.Q)
        e.init(I.Q)
        ids, dists = e.query(q[:I.Q])
        out = dict(ids=ids, dists=dists, counters=e.query_counters(I.Q), stats=e.stats())
        out["log"], out["cnt"] = e.candidate_log(I.Q, I.L)
        e.free()
        return out
    with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1) as e:
        e.load_index(ix)
        assert e.rows_pad() == I.N_PAD
        e.rows_slice(0, 100)                                               # given up for this load ...
        assert e.rows_pad() == 0
        e.unload()
        e.load_index(ix)                                                   # ... and decided anew by the next
        assert e.rows_pad() == I.N_PAD
        got = search(e)
        same_run(got, plain)
        check_sources(got, I.Q, I.N_PAD, SPARE)
        e.unload()
        e.set_option("rows_pad", 0)                                        # the same engine without: nothing of the padded load is left in its state
        e.load_index(ix)
        assert e.rows_pad() == 0
        got = search(e)
        same_run(got, plain)
        check_sources(got, I.Q, 0, SPARE)
        e.unload()


def test_environment_preset(libbang, monkeypatch, small_f32):
    import bang_amd
    ix, _ = I.index()
    monkeypatch.setenv("BANG_ROWS_HBM_SPARE_ROWS", str(SPARE))
    monkeypatch.setenv("BANG_ROWS_PAD", "0")
    with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1) as e:
        e.load_index(ix)
        assert e.rows_pad() == 0
        e.unload()
    monkeypatch.setenv("BANG_ROWS_PAD", "7")                               # clamped to 1 = forced: a layout without usable padding is refused by name

    def forced():
        with bang_amd.Engine("float", graph=GRAPH_HOST, pull=1) as e:
            e.load_index(small_f32[0])
    _refused(forced)
    with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1) as e:
        e.load_index(ix)
        assert e.rows_pad() == I.N_PAD
        e.unload()


def test_code_readers_see_the_same_codes(libbang):
    """bang_k_pqdist_stream on a table whose padding holds rows returns the bits it returns with the padding zero (and the oracle's)"""
    from bang_amd import binding as B
    from bang_amd.binding import IterState
    from oracle import oracle as O
    ix, q = I.index()
    orc = O.Oracle(ix)
    nq = 128
    qq = np.ascontiguousarray(q[:nq])
    rows = np.full((ix.N, 64), 0xFFFFFFFF, np.uint32)
    keep = np.arange(ix.R)[None, :] < ix.degrees()[:, None]
    rows[:, :ix.R][keep] = ix.adjacency()[keep]
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 65, nq).astype(np.uint32)
    cnt[:2] = (64, 1)
    nb = np.zeros((nq, B.NBR_STRIDE), np.uint32)
    for i in range(nq):
        nb[i, :cnt[i]] = rng.choice(ix.N, cnt[i], replace=False)
    got = []
    for table in (I.padded_table(ix.codes, rows, 0), I.padded_table(ix.codes, rows, I.N_PAD)):
        st = IterState(ix, qq, 16, ragged=True)
        st.d_nbrs.upload(nb)
        st.d_cnt.upload(cnt)
        st.d_dist.zero()
        p = st.params()
        d_tab = B.DeviceBuffer.from_numpy(table, slack=256)
        p.d_codes, p.code_stride = d_tab.ptr, 128
        B._check(B.lib().bang_k_pqdist_stream(C.byref(p), None), "bang_k_pqdist_stream")
        B.sync()
        got.append(st.nbrs()[2].copy())
        d_tab.free()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    for i in (0, 1, 17, nq - 1):
        want = orc.pqdist(orc.lut_build(qq[i]), nb[i, :cnt[i]])
        assert np.array_equal(got[1][i, :cnt[i]].view(np.uint32), want.view(np.uint32)), i


def _refused(build):
    import bang_amd
    with pytest.raises(bang_amd.BangError) as ei:
        build()
    assert "rows_pad" in str(ei.value), str(ei.value)


def test_forced_where_it_cannot_work_is_refused_by_name(libbang, monkeypatch, small_f32):
    import bang_amd
    ix, q = I.index()
    monkeypatch.setenv("BANG_ROWS_HBM_MAX_ROWS", str(I.N_COPY))

    def with_options(**opts):
        def build():
            with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1, rows_pad=1, **opts) as e:
                e.load_index(ix)
                assert e.rows_pad() == I.N_PAD
                e.set_searchparams(I.K, I.L)
                try:
                    e.alloc(I.Q)
                finally:
                    e.unload()
        return build
    _refused(with_options(walker=1))
    _refused(with_options(distance=1))
    _refused(with_options(persistent=0))

    def other_layout():                                   # 32 chunks of 4 dims: the code lines have no padding the kernel reads
        ix32 = small_f32[0]
        with bang_amd.Engine("float", graph=GRAPH_HOST, pull=1, rows_pad=1) as e:
            e.load_index(ix32)
    _refused(other_layout)

    def no_pull_mode(**opts):
        def build():
            with bang_amd.Engine("uint8", rows_pad=1, **opts) as e:
                e.load_index(ix)
        return build
    _refused(no_pull_mode(graph=1))                       # graph in HBM
    _refused(no_pull_mode(graph=GRAPH_HOST, pull=0))      # the walker serves the rows

    def peer_rows():
        with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1, rows_pad=1) as e:
            e.load_index(ix)
            try:
                e.rows_slice(0, 100)
            finally:
                e.unload()
    _refused(peer_rows)
    # ... and the same engine options without the force run as ever
    with bang_amd.Engine("uint8", graph=GRAPH_HOST, pull=1, rows_pad=0, distance=1) as e:
        e.load_index(ix)
        e.set_searchparams(I.K, I.L)
        e.alloc(I.Q)
        e.free()
        e.unload()
