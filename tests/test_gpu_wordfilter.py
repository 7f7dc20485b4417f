"""The word-local visited filter (option "filter_layout" = 1, search_wf_kernel of csrc/bang_search.hip) on a GPU: ids, distance bits and the four
per-query counters against the `word` composition of tests/wordfilter_reference.py -- on the crafted inputs of tests/wordfilter_inputs.py, where
the two layouts give DIFFERENT answers (asserted here too: an engine that ignored the option would fail), and on the ordinary fixtures, where
they agree.  Forms: graph in HBM; rows pulled from host memory with no, a partial and a full HBM copy; both forms of the speculative row
request; the filter summary on for every iteration and for the first only; the re-rank fused and launched; MIPS; one wave running 70 queries in
turn; every compiled instance on the layout list of tests/instance_inputs.py; the refusals; the CLI."""
import os
import subprocess

import numpy as np
import pytest

import base_forms as F
import edge_inputs as E
import instance_inputs as I
import wordfilter_inputs as WI
import wordfilter_reference as W

pytestmark = pytest.mark.gpu

K = 10
_REF = {}


def _ref(key, ix, q, L, layout="word", mips=False):
    """The CPU reference, once per (input, queries, L, layout)."""
    key = (key, q.shape[0], L, layout, mips)
    if key not in _REF:
        _REF[key] = W.Reference(ix).search(q, K, L, layout, mips)
    return _REF[key]


def _word_engine(ix, form, monkeypatch, **more):
    return F.open_engine(ix, form, monkeypatch, filter_layout=1, **more)


def _check(e, form, ix, q, L, want, code_stride=None):
    F.assert_same(F.run(e, form, q, K, L), want, form)
    s = F.assert_form(e, form, ix, q.shape[0], L, code_stride=code_stride)
    assert s["filter_layout"] == 1, s
    e.free()
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the crafted inputs: the layouts part, and the engine follows the one asked for
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("self_fused", "self_launch", "pull_host"))
@pytest.mark.parametrize("name", list(WI.INPUTS))
def test_crafted_inputs(name, form, monkeypatch):
    inp = WI.INPUTS[name]()
    split = _ref(name, inp.ix, inp.q, WI.L_TRACE, "split")
    word = _ref(name, inp.ix, inp.q, WI.L_TRACE)
    assert not np.array_equal(split[2], word[2])                          # (the point of the input: asserted on the CPU in test_wordfilter_mode.py)
    with _word_engine(inp.ix, form, monkeypatch) as e:
        for L in (WI.L_TRACE, 37):
            _check(e, form, inp.ix, inp.q, L, _ref(name, inp.ix, inp.q, L))
        e.unload()


@pytest.mark.parametrize("summ_iters", ("-1", "1"))
@pytest.mark.parametrize("name", list(WI.INPUTS))
def test_filter_summary_on_every_iteration_and_on_the_first_only(name, summ_iters, monkeypatch):
    """BANG_SUMM_ITERS: with the summary a word it knows untouched is not loaded and a survivor's store is its mask alone -- two survivors of one
    row in one word, and the 65th seed id beside one of the first 64, must still both land."""
    inp = WI.INPUTS[name]()
    monkeypatch.setenv("BANG_SUMM_ITERS", summ_iters)
    with _word_engine(inp.ix, "self_fused", monkeypatch) as e:
        s = _check(e, "self_fused", inp.ix, inp.q, WI.L_TRACE, _ref(name, inp.ix, inp.q, WI.L_TRACE))
        assert s["filter_loads_skipped"] > 0
        e.unload()


def test_kernel_level_entry_on_a_crafted_input():
    """IterState.run_search_wf -> bang_k_search_wf: candidate log, counters and iterations of the `word` reference; run_search() beside it gives
    those of the split layout."""
    import bang_amd
    inp = WI.word_drops()
    ref = W.Reference(inp.ix)
    for layout, run in (("word", "run_search_wf"), ("split", "run_search")):
        st = bang_amd.IterState(inp.ix, inp.q, WI.L_TRACE, device_graph=True)
        iters = getattr(st, run)()
        cnt, ids, _ = st.candidates()
        qs = st.d_qstats.download(np.uint32, (inp.q.shape[0], 2))
        for i in range(inp.q.shape[0]):
            log = []
            _, _, (it, nc, evals, fetched) = ref.search_one(inp.q[i], K, WI.L_TRACE, layout, log=log)
            assert (int(iters[i]), int(cnt[i]), int(qs[i, 0]), int(qs[i, 1])) == (it, nc, evals, fetched), (layout, i)
            assert ids[i, :nc].tolist() == log, (layout, i)


# ---------------------------------------------------------------------------------------------------------------------
# the ordinary fixtures, every L; the iteration cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (10, 37, 152))
@pytest.mark.parametrize("fixture", ("small_u8", "small_deep", "small_f32"))
def test_fixtures_graph_in_hbm(request, fixture, L, monkeypatch):
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = q[:16]
    with _word_engine(ix, "self_fused", monkeypatch) as e:
        _check(e, "self_fused", ix, q, L, _ref(fixture, ix, q, L))
        e.unload()


def test_chain_runs_to_the_iteration_cap(monkeypatch):
    ix, q = E.chain()
    want = _ref("chain", ix, q, 152)
    assert want[2][0, 0] == 152 + 49                                      # the walk ends at the cap
    for form in ("self_fused", "pull_host"):
        with _word_engine(ix, form, monkeypatch) as e:
            _check(e, form, ix, q, 152, want)
            e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# pulled rows; the speculative row request; MIPS; launch shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("pull_host", "pull_part", "pull_slice"))
@pytest.mark.parametrize("name", ("small_u8", "word_drops"))
def test_pulled_rows(request, name, form, monkeypatch):
    """graph = host, rows pulled by the kernel: all over PCIe; the first third in HBM (BANG_ROWS_HBM_MAX_ROWS); all in HBM (rows_slice)."""
    if name == "small_u8":
        ix, q, _, _ = request.getfixturevalue(name)
        q = q[:16]
    else:
        inp = WI.word_drops()
        ix, q = inp.ix, inp.q
    if form == "pull_slice":
        e = _word_engine(ix, "pull_host", monkeypatch)
        e.rows_slice(0, ix.N)
    else:
        e = _word_engine(ix, form, monkeypatch)
    with e:
        for L in (10, 37):
            _check(e, "pull_hbm" if form == "pull_slice" else form, ix, q, L, _ref(name, ix, q, L))
        e.unload()


@pytest.mark.parametrize("spec_rows", ("1", "2"))
@pytest.mark.parametrize("fixture", ("small_u8", "small_deep"))
def test_speculative_row_request_on_and_off(request, fixture, spec_rows, monkeypatch):
    """BANG_SPEC_ROWS on the 70- and 74-chunk layouts, the ones with SPEC instances: same results either way."""
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = q[:16]
    monkeypatch.setenv("BANG_SPEC_ROWS", spec_rows)
    for form in ("self_fused", "pull_host"):
        with _word_engine(ix, form, monkeypatch) as e:
            _check(e, form, ix, q, 37, _ref(fixture, ix, q, 37))
            e.unload()


def test_mips(small_f32):
    import bang_amd
    ix, q, _, _ = small_f32
    q1 = np.ascontiguousarray(q[:16, :-1])
    want = _ref("small_f32", ix, q1, 37, mips=True)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, filter_layout=bang_amd.FILTER_WORD) as e:
        e.load_index(ix)
        e.set_searchparams(K, 37, bang_amd.DIST_MIPS)
        e.alloc(16)
        e.init(16)
        ids, d = e.query(q1)
        F.assert_same((ids, d, e.query_counters(16)), want)
        s = e.stats()
        assert s["filter_layout"] == 1 and s["search_kernel"] == 1 and s["rerank_fused"] == 0, s


@pytest.mark.parametrize("form", ("self_fused", "pull_host"))
def test_batches_of_one_three_and_seventy_on_one_wave(form, monkeypatch):
    """Q = 1 and Q = 3 on one allocation; then 70 queries -- the crafted input's six, repeated -- with one workgroup of one wave, which runs them
    in turn: filter-summary or claim-table state left over from the query before would show in the one after."""
    inp = WI.word_drops()
    ref = _ref("word_drops", inp.ix, inp.q, WI.L_TRACE)
    with _word_engine(inp.ix, form, monkeypatch) as e:
        e.set_searchparams(K, WI.L_TRACE)
        e.alloc(3)
        for nb in (1, 3):
            e.init(nb)
            ids, d = e.query(inp.q[:nb])
            F.assert_same((ids, d, e.query_counters(nb)), (ref[0][:nb], np.ascontiguousarray(ref[1][:, :nb]), ref[2][:nb]), form)
        e.free()
        rep = np.arange(70) % inp.q.shape[0]
        q70 = np.ascontiguousarray(inp.q[rep])
        monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
        monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
        _check(e, form, inp.ix, q70, WI.L_TRACE, (ref[0][rep], np.ascontiguousarray(ref[1][:, rep]), ref[2][rep]))
        e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# every compiled instance of the new build
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", I.ENTRIES, ids=I.entry_id)
def test_every_instance(entry, monkeypatch):
    """bang_k_search_wf on each pivot layout of search_dispatch, code rows dword-aligned and not (the engine reports the stride it was asked
    for); the 70- and 74-chunk layouts in both forms of the speculative row request."""
    ix, q = I.entry_index(entry)
    want = _ref(I.shape_of(entry), ix, q, 37)
    for spec in (("1", "2") if entry.key in (218, 219) else ("0",)):
        monkeypatch.setenv("BANG_SPEC_ROWS", spec)
        form = "self_fused" if F.fusable(ix.dtype, ix.D, ix.entry_len) else "self_launch"
        with _word_engine(ix, form, monkeypatch, **I.options_of(entry)) as e:
            _check(e, form, ix, q, 37, want, code_stride=I.stride_of(entry))
            e.unload()


# ---------------------------------------------------------------------------------------------------------------------
# the default, the refusals, the CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_split_layout_is_reported_and_is_the_oracle(small_u8, monkeypatch):
    from oracle import oracle as O
    ix, q, _, _ = small_u8
    q = q[:16]
    want = O.Oracle(ix).search(q, K, 37, with_stats=True)
    for more in (dict(), dict(filter_layout=0)):
        with F.open_engine(ix, "self_fused", monkeypatch, **more) as e:
            F.assert_same(F.run(e, "self_fused", q, K, 37), want)
            assert e.stats()["filter_layout"] == 0
            e.free()
            e.unload()
    inp = WI.word_drops()                                                  # ... also where the word layout would answer differently
    with F.open_engine(inp.ix, "self_fused", monkeypatch, filter_layout=0) as e:
        F.assert_same(F.run(e, "self_fused", inp.q, K, WI.L_TRACE), _ref("word_drops", inp.ix, inp.q, WI.L_TRACE, "split"))
        assert e.stats()["filter_layout"] == 0
        e.free()
        e.unload()


REFUSED = {
    "search_0":     dict(graph=1, search=0),
    "persistent_0": dict(graph=1, persistent=0),
    "lut_path":     dict(graph=1, pq=1, search=1),
    "walker":       dict(graph=0, pull=1, walker=1),
    "host_paced":   dict(graph=0, pull=0),
    "exact":        dict(graph=1, distance=1),
    "beam":         dict(graph=1, distance=1, beam=2),
    "inmemory":     dict(graph=1, semantics=1),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_name_the_option(case, small_i8):
    """Every configuration that does not end on the self-paced search kernel is refused at bang_alloc, with filter_layout in the message: there
    is no silent fallback to the split layout."""
    import bang_amd
    ix, q, _, _ = small_i8
    with bang_amd.Engine(ix.dtype, filter_layout=1, **REFUSED[case]) as e:
        e.load_index(ix)
        e.set_searchparams(K, 24)
        with pytest.raises(bang_amd.BangError, match="filter_layout"):
            e.alloc(8)


@pytest.mark.timeout(400, method="thread")
def test_cli_reports_the_reference_recall(small_i8, tmp_path):
    """BANG_FILTER_LAYOUT=word BANG_GRAPH=device bang_search (interactive L) prints its usual table; its recall at each L is the reference's."""
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
    env = dict(os.environ, BANG_FILTER_LAYOUT="word", BANG_GRAPH="device", BANG_DEBUG="1")
    out = subprocess.run([exe, prefix, str(tmp_path / "q.bin"), str(tmp_path / "gt.bin"), str(q.shape[0]), "10", "int8", "l2"],
                         input="".join(f"{L}\ny\n" for L in Ls[:-1]) + f"{Ls[-1]}\nn\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "filter_layout=1" in out.stderr                                # (BANG_DEBUG: what bang_alloc resolved)
    rows = [l.split("\t") for l in out.stdout.splitlines() if l[:1].isdigit() and l.count("\t") == 3]
    assert "10-r@10" in out.stdout and sorted({int(r[0]) for r in rows}) == list(Ls)
    for L in Ls:
        ids, _, _ = _ref("small_i8", ix, q, L)
        want = f"{float(np.float32(O.recall(gt_i, gt_d, ids, 10))):.2f}"
        got = [r[3].strip() for r in rows if int(r[0]) == L]
        assert len(got) == 5 and all(g == want for g in got), (L, got, want)
