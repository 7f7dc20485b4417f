"""The forms in which the engine runs the BANG_Base PQ walk, as engine options plus what bang_get_stats must then report.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest), shared by tests/test_gpu_search_instances.py and tests/test_gpu_base_edges.py.  One
source, search_kernel of csrc/bang_search.hip, is compiled as the self-paced form with the graph in HBM, the pulled-rows form (graph in host RAM,
the kernel reads 256-byte adjacency rows from pinned host memory or from their HBM copy) and the host-paced form (walker threads serve the rows);
the launch-per-iteration loop is the older form beside it.  Every form returns the bits of oracle.Oracle.search.

    GROUPS                     group -> forms; a test case is one (input, group), an engine one (input, form)
    forms_of()                 the forms of a group on a layout that has a search-kernel instance;  LUT_FORMS for a layout on the LUT path
    open_engine()              a loaded engine in a form;  run();  assert_same()
    host_paced_waves()         does LDS hold the host-paced form on a layout?  (host code; asserted by the CPU files for every input)
    assert_form()              the statistics that prove the form asked for is the one that ran
"""
from __future__ import annotations

import numpy as np
import pytest

GROUPS = {
    "self":       ("self_fused", "self_launch"),                  # graph in HBM, ONE launch; the re-rank inside it / in a launch of its own
    "pulled":     ("pull_host", "pull_part", "pull_hbm"),         # rows in pinned host memory; the first third also in HBM; all of them in HBM
    "host_paced": ("walker_graph", "walker_rows"),                # walker threads read graph entries / the pull rows
    "loop":       ("loop",),                                      # graph in HBM, a front and a back launch per iteration
}
OPTIONS = {
    "self_fused":   dict(graph=1, search=1, fuse_rerank=1),
    "self_launch":  dict(graph=1, search=1, fuse_rerank=0),
    "pull_host":    dict(graph=0, pull=1),
    "pull_part":    dict(graph=0, pull=1, rows_hbm=64),
    "pull_hbm":     dict(graph=0, pull=1, rows_hbm=64),
    "walker_graph": dict(graph=0, pull=0, search=1),
    "walker_rows":  dict(graph=0, pull=1, walker=1),
    "loop":         dict(graph=1, search=0),
    # LUT-path layouts (psz == 0), graph in HBM: the loop they keep by default, and search_lut_kernel where search = 1 asks for it
    "lut_loop":     dict(graph=1),
    "lut_kernel":   dict(graph=1, search=1),
}
LUT_FORMS = ("lut_loop", "lut_kernel")
EDGE_MAX_L = 37                   # the longest worklist of tests/test_gpu_base_edges.py on a layout with a search-kernel instance
MIN_ROWS_HBM = 64                  # bang_load.cpp cache_rows_in_hbm: a copy of fewer rows is not made
NO_BAR = "device memory is not CPU-writable here (no large BAR): the host-paced search kernel is not used"


def tsize(dtype: str) -> int:
    return 4 if dtype == "float" else 1


def fusable(dtype: str, D: int, vec_stride: int) -> bool:
    """bang_search_can_rerank (csrc/bang_search_host.cpp) restated, so that a parameter list can be made without the library;
    tests/test_instance_inputs.py pins it to the library's answer."""
    if vec_stride % 4 or D > 256:
        return False
    if dtype == "float":
        return D >= 4 and D % 4 == 0
    G = D >> 4
    return D >= 16 and D % 16 == 0 and (G & (G - 1)) == 0


def forms_of(group: str, dtype: str, D: int, R: int, N: int):
    """The forms of a group that differ on this layout: without a layout the fused re-rank evaluates there is one self-paced form, and an index
    of fewer than 3 x 64 nodes has no partial HBM copy of its rows."""
    forms = GROUPS[group]
    if group == "self" and not fusable(dtype, D, D * tsize(dtype) + 4 + 4 * R):
        forms = ("self_launch",)
    if group == "pulled" and N // 3 < MIN_ROWS_HBM:
        forms = ("pull_host", "pull_hbm")
    return forms


def reports_iterations(form: str) -> bool:
    return form not in ("loop", "lut_loop")


def open_engine(ix, form: str, monkeypatch, **more):
    """An engine with the index loaded in `form`.  pull_part: the test hook BANG_ROWS_HBM_MAX_ROWS (read at load) cuts the HBM copy to the first
    third of the rows.  pull_hbm on an index of fewer than 64 nodes: bang_rows_slice_e, which copies any number of rows."""
    import bang_amd
    e = bang_amd.Engine(ix.dtype, **dict(OPTIONS[form], **more))
    try:
        if form == "pull_part":
            monkeypatch.setenv("BANG_ROWS_HBM_MAX_ROWS", str(ix.N // 3))
        e.load_index(ix)
        if form == "pull_hbm" and ix.N < MIN_ROWS_HBM:
            e.rows_slice(0, ix.N)
    except BaseException:
        e.close()
        raise
    finally:
        if form == "pull_part":
            monkeypatch.delenv("BANG_ROWS_HBM_MAX_ROWS")
    return e


def run(e, form: str, q, k: int, L: int, Q=None):
    """set_searchparams + alloc + init + query -> (ids, dists, per-query counters).  The caller frees.  A host-paced form that reports
    search_kernel == 0 skips: device memory is not CPU-writable there -- the one skip of these files, and of this leg alone.  Nothing else leads
    to it: host_paced_waves() below is the other condition of bang_alloc, and the CPU files assert it for every input that comes here.  A
    refusal of bang_alloc is an error, never a skip."""
    e.set_searchparams(k, L)
    e.alloc(q.shape[0] if Q is None else Q)
    e.init(q.shape[0])
    ids, d = e.query(q)
    if form in GROUPS["host_paced"] and not e.stats()["search_kernel"]:
        pytest.skip(NO_BAR)
    return ids, d, e.query_counters(q.shape[0])


def host_paced_waves(ix, L: int, pq_ragged: int = 1) -> int:
    """Waves per workgroup of the host-paced search kernel on this layout at this L, decided as bang_alloc.cpp and bang_search_geometry decide it
    (host code: no GPU needed); 0 = the engine would decline the form for want of LDS, or the layout is on the LUT path."""
    import ctypes as C
    from bang_amd import binding as B
    lib = B.lib()
    u32 = C.c_uint32
    lib.bang_search_supported.argtypes = [u32] * 4
    lib.bang_ragged_supported.argtypes = [u32] * 4
    psz, mp = B.pq_layout(ix.chunk_off, ix.D, ix.m)
    if psz == 0:
        return 0
    nhi = 0
    if psz == 2 and pq_ragged:                                      # bang_load.cpp: the exact-size table, where an instance exists for it
        nhi, _ = B.pack_pivots_ragged(ix.pivots, ix.chunk_off, ix.D, ix.m, mp)
        if not (nhi and lib.bang_ragged_supported(psz, mp, nhi, ix.m)):
            nhi = 0
    w_pad = lib.bang_search_supported(psz, mp, 0, L)
    w_rag = lib.bang_search_supported(psz, mp, nhi, L) if nhi else 0
    if max(w_pad, w_rag) < 4:                                       # option search = auto (form walker_rows) asks for 4, search = 1 for 1
        return 0
    wgs, waves, nctx, gs = u32(0), u32(0), u32(0), u32(0)
    rc = lib.bang_search_geometry(u32(psz), u32(mp), u32(nhi if w_rag > w_pad else 0), u32(L), u32(1 << 20), u32(0), u32(0), C.c_int(1),
                                  C.byref(wgs), C.byref(waves), C.byref(nctx), C.byref(gs))
    return int(waves.value) if rc == 0 else 0


def assert_same(got, want, form: str = "self_fused"):
    ids, d, st = got
    ids_r, d_r, st_r = want
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(d.view(np.uint32), d_r.view(np.uint32))
    if reports_iterations(form):
        assert np.array_equal(st, st_r)                       # iterations, candidates, dist_evals, fetched
    else:
        assert np.array_equal(st[:, 1:], st_r[:, 1:])         # (the loop reports no per-query iterations)


def assert_form(e, form: str, ix, Q: int, L: int, code_stride=None):
    """bang_get_stats after a query: the form asked for is the one that ran."""
    s = e.stats()
    if code_stride is not None:
        assert s["code_stride"] == code_stride, s
    vb = ix.D * tsize(ix.dtype)
    if form in GROUPS["self"]:
        assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["graph_pull"] == 0 and s["graph_mode"] == 1, s
        assert s["rerank_fused"] == int(form == "self_fused" and fusable(ix.dtype, ix.D, ix.entry_len)), s
    elif form in GROUPS["pulled"]:
        assert s["graph_pull"] == 1 and s["search_kernel"] == 1 and s["front_launches"] == 1 and s["vectors_on_device"] == 1, s
        assert s["walker_threads"] == 0 and s["rerank_fused"] == int(fusable(ix.dtype, ix.D, vb)), s
        n_hbm = {"pull_host": 0, "pull_part": ix.N // 3, "pull_hbm": ix.N}[form]
        assert s["rows_in_hbm"] == n_hbm, s
        c_ids, c_cnt = e.candidate_log(Q, L)
        own = sum(int((c_ids[i, 1:c_cnt[i]] < n_hbm).sum()) for i in range(Q))          # expanded nodes whose row sits in this GPU's HBM
        assert s["rows_from_own_hbm"] == own and s["rows_from_peer"] == 0, s
        assert s["pulled_bytes"] == 256 * (int(s["candidates"]) - Q - own), s
        if form == "pull_hbm":
            assert s["pulled_bytes"] == 0, s
    elif form in GROUPS["host_paced"]:
        assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["graph_pull"] == 0 and s["pacing_groups"] > 0, s
        assert s["walker_rows"] == int(form == "walker_rows"), s
    elif form == "loop" or form == "lut_loop":
        assert s["search_kernel"] == 0 and s["persistent"] == 0, s
    elif form == "lut_kernel":
        assert s["search_kernel"] == 1 and s["front_launches"] == 1 and s["rerank_fused"] == 0, s
    else:
        raise ValueError(form)
    return s
