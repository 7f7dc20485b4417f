"""The host side of the query-resident search kernel (csrc/bang_search_host.cpp, no HIP call) without a GPU.

* Its pure functions -- PQ layout, pivot packing, which instances exist, the launch geometry -- answer what tests/golden/search_host_sweep.json
  recorded from the library of the commit before they moved there (tests/golden/make_search_host_golden.py), error codes included.
* A launch: csrc/bang_search_host.cpp + tests/search_host_main.cpp are built with -fsanitize=address,undefined and run as a program (no Python runs
  under a sanitizer).  The main stubs the CU count and the instance dispatch, which prints the SearchArgs it was handed.  The three launch policies,
  the grid and the LDS formula are restated below from the comments of the source and compared with what was printed, on both sides of every
  threshold; every refusal of the argument checks is reached with its message."""
import ctypes as C
import importlib.util
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
LDS_BYTES = 160 * 1024
ALWAYS = 0xFFFFFFFF


def _maker():
    spec = importlib.util.spec_from_file_location("make_search_host_golden", os.path.join(GOLDEN, "make_search_host_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_library_reproduces_the_recorded_sweep(libbang):
    M = _maker()
    want = json.load(open(M.OUT))
    libbang.bang_num_cus.restype = C.c_int
    assert libbang.bang_num_cus() == want["cus"], "the geometry rows were recorded for 256 CUs (no device, or an MI355X)"
    rows = M.sweep(libbang)
    got = M.record(rows)
    assert sorted(got) == sorted(want)
    assert sum(len(v["answers"]) for v in want.values() if isinstance(v, dict)) > 4000
    for name, n in M.NARGS.items():
        assert got[name]["questions"] == want[name]["questions"] and len(got[name]["answers"]) == len(want[name]["answers"]), name
        for row, g, w in zip(rows[name], got[name]["answers"], want[name]["answers"]):
            assert g == w, (name, row[:n], g, w)
    # ... and the sweep holds what it is there for: every layout, both exact-size tables, answers of every kind
    geometry = rows["search_geometry"]
    assert {(psz, 4 * ndw, 0) for psz, ndw in M.LAYOUTS} | {(2, 72, 58), (2, 76, 22)} <= {tuple(r[:3]) for r in geometry if r[10] != ERR_ARG}
    assert {r[10] for r in geometry} == {OK, ERR_ARG, ERR_UNSUPPORTED}
    assert {(r[7], r[8], r[9], r[5], r[6]) for r in geometry} >= {(1, *t[:2], *t[2]) for t in itertools.product(M.NCTX, M.GROUP_WAVES, M.CAPS)}
    for name in ("ragged_supported", "search_can_rerank", "search_wf_has_instance", "search_inmem_has_instance"):
        assert set(want[name]["answers"]) == {0, 1}, name


# ---------------------------------------------------------------------------------------------------------------------
# a launch, under sanitizers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("search_host") / "search_host_san")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "bang_search_host.cpp"),
           os.path.join(ROOT, "tests", "search_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run_launches(exe, cus, lines):
    """one launch per line (tests/search_host_main.cpp) -> one dict per launch"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("BANG_SEARCH_PRIO", None)
    out = subprocess.run([exe, str(cus)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    got = []
    for text in out.stdout.splitlines():
        head, _, err = text.partition(" err=")
        d = {k: int(v) for k, v in (t.split("=") for t in head.split())}
        d["err"] = err
        got.append(d)
    assert len(got) == len(lines)
    return got


# The layouts, restated (csrc/bang_search_args.h): long code rows (>= 64 chunks, 16+ dwords) run in workgroups of 768 threads with 256 words of
# scratch per wave, the others in 1024 threads with 144; the pivot table; a wave's LDS; what fits beside the table
LAYOUTS = ((1, 8), (1, 16), (1, 24), (1, 32), (2, 8), (2, 16), (2, 18), (2, 19), (4, 4), (4, 8), (8, 2), (8, 4))
TABLES = [(psz, 4 * ndw, 0) for psz, ndw in LAYOUTS] + [(2, 72, 58), (2, 76, 22)]


def maxt(mp):
    return 768 if mp // 4 >= 16 else 1024


def pivot_floats(psz, mp, nhi):
    return ((nhi * 512 + (mp - nhi) * 256 + 3) & ~3) + 4 if psz == 2 and nhi else mp * 256 * psz


def wl_words(L):
    return (2 * L + (L + 3) // 4 + 3) & ~3


def wave_words(mp, L):
    return wl_words(L) + (256 if mp // 4 >= 16 else 144)


def waves_that_fit(psz, mp, nhi, L, host_paced):
    room = LDS_BYTES - (2048 if host_paced else 0) - 4 * pivot_floats(psz, mp, nhi)
    return min(room // (4 * wave_words(mp, L)), maxt(mp) // 64)


def expected(entry, form, psz, mp, nhi, L, Q, cus, spec_rows, summ_iters, prio):
    """What the dispatch must be handed.  One workgroup per CU at most; no more waves than a workgroup's share of the batch; a self-paced batch of one
    to two wave-fulls runs as two equal rounds.  Filter summary: off (1) up to 5 queries per CU.  Wave priority: on (3) up to 10 queries per CU;
    BANG_SEARCH_PRIO = 0 / 1 / 2 / 3 forces 0 / 3 / 2 / 1.  spec_rows: 70- / 74-chunk layouts only, never semantics = 1 or host-paced; auto = on where
    the rows are pulled, and up to 8 queries per CU."""
    host_paced = form == "host"
    fit = waves_that_fit(psz, mp, nhi, L, host_paced)
    grid = min(Q, cus)
    per = -(-Q // grid)
    waves = per if per < fit else (per + 1) // 2 if (not host_paced and fit < per <= 2 * fit) else fit
    e = dict(rc=OK, part={"search": 0, "inmem": 2, "wf": 4}[entry], grid=grid, block=64 * waves, nctx=1, gs=min(8, waves) if host_paced else waves,
             wl_words=wl_words(L), wave_words=wave_words(mp, L), lds_piv_floats=pivot_floats(psz, mp, nhi), cap_iter=L + 49, err="")
    e["lds"] = 4 * e["lds_piv_floats"] + 4 * waves * e["wave_words"] + (2048 if host_paced else 0)
    e["summ_iters"] = e["summ_iters_p"] = summ_iters if summ_iters else (1 if per <= 5 else ALWAYS)
    e["prio"] = {"0": 0, "1": 3, "2": 2, "3": 1}[prio] if prio != "-" else (3 if per <= 10 else 0)
    can_spec = mp in (72, 76) and entry != "inmem" and not host_paced
    e["spec_rows"] = 1 if can_spec and (spec_rows == 1 or (spec_rows == 0 and (form == "pulled" or per <= 8))) else 2
    return e


FORMS = {"hbm": "", "pulled": " row_layout=1", "host": " d_graph=0"}
ENTRY_FORMS = (("search", "hbm"), ("search", "pulled"), ("search", "host"), ("wf", "hbm"), ("wf", "pulled"), ("inmem", "hbm"))
KNOBS = [(s, i, "-") for s in (0, 1, 2) for i in (0, 3)] + [(0, 0, prio) for prio in "0123"]      # (spec_rows, summ_iters, BANG_SEARCH_PRIO)


@pytest.mark.parametrize("cus", [256, 8])
def test_launch_policies_geometry_and_lds(host_exe, cus):
    L = 152
    cases = []
    for (psz, mp, nhi), (entry, form) in itertools.product(TABLES, ENTRY_FORMS):
        fit = waves_that_fit(psz, mp, nhi, L, False)
        assert fit >= 3, (psz, mp, nhi)
        qs = {1, cus - 1, cus * fit, cus * fit + 1, 2 * cus * fit, 2 * cus * fit + 1} | {k * cus + d for k in (5, 8, 10) for d in (0, 1)}
        cases += [(entry, form, psz, mp, nhi, L, Q, cus) + knobs for Q in sorted(qs) for knobs in KNOBS]
    lines = [f"{entry} psz={psz} mp={mp} pq_nhi={nhi} m={mp - 2} L={L} cap_iter={L + 49} Q={Q} spec_rows={spec} summ_iters={summ} prio={prio}" + FORMS[form]
             for entry, form, psz, mp, nhi, L, Q, _, spec, summ, prio in cases]
    seen = {"spec_rows": set(), "prio": set(), "summ_iters": set(), "rounds": set()}
    for case, got in zip(cases, run_launches(host_exe, cus, lines)):
        assert got == expected(*case), case
        assert got["block"] <= maxt(case[3]) and got["lds"] <= LDS_BYTES, case
        for k in ("spec_rows", "prio", "summ_iters"):
            seen[k].add(got[k])
        seen["rounds"].add(got["block"] // 64 < waves_that_fit(*case[2:6], case[1] == "host"))
    assert seen == {"spec_rows": {1, 2}, "prio": {0, 1, 2, 3}, "summ_iters": {1, 3, ALWAYS}, "rounds": {True, False}}


GOOD_RR = "rr_queries=0x10000 rr_vec_base=0x20000 rr_vec_stride=388 rr_ids_out=0x30000 rr_dists_out=0x40000 rr_dtype=0 rr_D=128 rr_k=10 rr_q0=0 rr_Q_total=100"
REFUSALS = (
    [("search", kv, ERR_ARG, "bad R/L/m") for kv in ("R=0", "R=65", "L=0", "L=513", "m=0")] +
    [("search", kv, ERR_UNSUPPORTED, "the search kernel needs the LDS-resident pivot layout") for kv in ("psz=0", "mp=68", "mp=74")] +
    [("search", f"{buf}=0", ERR_ARG, "null buffer")
     for buf in ("d_codes", "d_pivots_packed", "d_qc", "d_seed", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query")] +
    [("search", f"d_graph=0 {buf}=0", ERR_ARG, "host-paced search kernel: null pacing buffer") for buf in ("d_rows", "d_ctl", "h_done", "h_parents")] +
    [("search", f"d_graph=0 ship_vectors=1 {kv}", ERR_ARG, "host-paced search kernel: null pacing buffer") for kv in ("h_pub_c=0x100", "h_pub_q=0x100")] +
    [("inmem", kv, ERR_UNSUPPORTED, "semantics = 1: the graph entries must be in HBM (d_graph, row_layout 0)") for kv in ("d_graph=0", "row_layout=1")] +
    [("search", kv, ERR_ARG, "bad pq_nhi") for kv in ("psz=1 mp=32 m=30 pq_nhi=5", "pq_nhi=73")] +
    [("search", "cap_iter=0", ERR_ARG, "bad iteration cap"), ("search", "cap_iter=202", ERR_ARG, "bad iteration cap"),
     ("wf", "cap_iter=202", ERR_ARG, "bad iteration cap"), ("inmem", "cap_iter=272", ERR_ARG, "bad iteration cap")] +
    [("search", GOOD_RR + " d_graph=0", ERR_ARG, "the fused re-rank belongs to the self-paced form")] +
    [(entry, GOOD_RR + " " + kv, ERR_ARG, "fused re-rank: bad arguments / unsupported vector layout")
     for entry in ("search", "inmem") for kv in ("rr_vec_base=0", "rr_ids_out=0", "rr_dists_out=0", "rr_k=0", "rr_Q_total=99", "rr_q0=1", "rr_D=48",
                                                 "rr_vec_stride=390", "rr_vec_base=0x20002", "rr_queries=0x10002", "rr_dtype=3")] +
    [("wf", "d_graph=0", ERR_UNSUPPORTED, "filter_layout = 1: the word-local filter belongs to the self-paced form (d_graph: graph entries or pulled rows)")] +
    [("search", "mp=128 m=128", ERR_UNSUPPORTED, "pivot table + one wave's worklist do not fit LDS at L=152")] +
    [("null", "", ERR_ARG, "")]
)
ACCEPTED = (("search", "cap_iter=201", 0), ("inmem", "cap_iter=271", 2), ("wf", "", 4), ("search", GOOD_RR, 0), ("inmem", GOOD_RR, 2), ("wf", GOOD_RR, 4),
            ("search", "d_graph=0 ship_vectors=1 h_pub_q=0x100 h_pub_c=0x200", 0), ("search", "pq_nhi=58", 0))


def test_every_refusal_comes_with_its_code_and_message_and_no_dispatch(host_exe):
    got = run_launches(host_exe, 256, [f"{entry} {kv}" for entry, kv, _, _ in REFUSALS])
    for (entry, kv, rc, msg), g in zip(REFUSALS, got):
        assert (g["rc"], g["part"], g["err"]) == (rc, -1, msg), (entry, kv, g)
    got = run_launches(host_exe, 256, [f"{entry} {kv}" for entry, kv, _ in ACCEPTED] + ["search Q=0 d_codes=0", "inmem Q=0", "wf Q=0 d_graph=0"])
    for (entry, kv, part), g in zip(ACCEPTED, got):
        assert (g["rc"], g["part"], g["err"]) == (OK, part, ""), (entry, kv, g)
    for g in got[len(ACCEPTED):]:                                                # an empty batch: no check, no launch
        assert (g["rc"], g["part"], g["err"]) == (OK, -1, "")
