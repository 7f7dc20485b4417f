"""Every kernel's row addressing beyond 4 GiB: each case launches ONE kernel-level entry of include/bang_c.h on tables laid out at stretched
strides (tests/stretch_inputs.py: 640 rows 32 MiB apart, ids >= 128 beyond 4 GiB, ids >= 512 beyond 16 GiB, behind a zeroed lead-in of 2 GiB)
and compares with the CPU reference on the compact index bit for bit -- ids, distance bits, per-query iterations, d_qstats, the candidate log,
and d_abort == 0.  The stride does not enter the semantics, so a difference is a narrow `id * stride` (or the engine not handing the stride
on); tests/test_stretch_inputs.py proves on the CPU that a product wrapped at 2^32 or 2^34 changes every one of these answers.  The cases come
from stretch_inputs.CASES; the entries without a walk (K2 alone, the two vector-log forms of the re-rank, the fp16 conversion) follow.  At most
one stretched buffer of < 24 GiB is alive at a time and it is freed before the next case; a failed allocation fails the case ("box too small").
The 256-byte adjacency rows of the pulled forms have a fixed stride: their offsets beyond 4 GiB stay with tests/test_gpu_scale.py."""
import ctypes as C

import numpy as np
import pytest

import stretch_inputs as S
from test_f16_convert_host import convert  # noqa: F401  (the fixture: csrc/bang_f16.h compiled for the host)

pytestmark = pytest.mark.gpu
Q, K, L = S.Q, S.K, S.L
ROWS = L + 50


def _B():
    from bang_amd import binding as B
    return B


def _free(held):
    for b in held:
        b.free()


def _cases(*entries):
    cs = [c for c in S.CASES if c.entry in entries]
    return pytest.mark.parametrize("case", cs, ids=[S.case_id(c) for c in cs])


def _assert_results(ids, dists, w):
    assert np.array_equal(ids, w.ids)
    assert np.array_equal(np.asarray(dists).view(np.uint32), w.dists.view(np.uint32))


def _assert_walk(w, iters, cnt, log, qstats, abort):
    """per-query iterations, candidate count and log, d_qstats {distance evaluations, ids fetched}, d_abort"""
    assert np.array_equal(np.asarray(iters, np.int64), w.stats[:, 0])
    assert np.array_equal(np.asarray(cnt, np.int64), w.stats[:, 1])
    assert np.array_equal(np.asarray(qstats[:, 0], np.int64), w.stats[:, 2]) and np.array_equal(np.asarray(qstats[:, 1], np.int64), w.stats[:, 3])
    for i in range(Q):
        assert np.array_equal(log[i, :cnt[i]], w.logs[i]), i
    assert abort == 0


def _seed(ix):
    adj = ix.adjacency()[ix.medoid][: int(ix.degrees()[ix.medoid])]
    seed = np.zeros(2 + 65, dtype=np.uint32)
    seed[0], seed[1] = 1 + len(adj), ix.medoid
    seed[2:2 + len(adj)] = adj
    return seed


def _pull_rows(ix):
    """the 256-byte adjacency rows of the pulled forms: 64 ids, the unused slots 0xFFFFFFFF"""
    rows = np.full((ix.N, 64), 0xFFFFFFFF, np.uint32)
    keep = np.arange(ix.R)[None, :] < ix.degrees()[:, None]
    rows[:, :ix.R][keep] = ix.adjacency()[keep]
    return rows


def _f32_to_f16(B, d_src, d_dst, rows, D, src_stride, dst_stride, d_bad):
    fn = B.lib().bang_k_f32_to_f16
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    B._check(fn(d_src, d_dst, rows, D, src_stride, dst_stride, d_bad, None), "bang_k_f32_to_f16")
    B.sync()


# ------------------------------------------------------------------------------------------------------------------------ exact-distance kernels
@_cases("search_exact", "search_exact_beam")
def test_exact_distance_search(case):
    """bang_k_search_exact (its wide, pulled and fp16 instances) and bang_k_search_exact_beam: entry_len stretched where the graph entries are
    in HBM (row_layout 0), rr_vec_stride where the rows are pulled (row_layout 1: the rows in a device buffer, n_rows_hbm = N)."""
    B = _B()
    ix, q = S.get(case.input)
    opt = dict(case.opt)
    w = S.walk(case.input, case.mode)
    vb = ix.D * S.tsize(ix)
    held = []
    try:
        sp = B.SearchParams()
        if opt["layout"] == 0:
            stride = S.stride_for(case, "graph")
            big, ptr = S.stretched(ix.graph, stride)
            held.append(big)
            sp.d_graph, sp.entry_len = ptr, stride
        else:
            stride = S.stride_for(case, "vectors")
            rows = B.DeviceBuffer.from_numpy(_pull_rows(ix), slack=256)
            held.append(rows)
            if opt.get("f16"):                                # the table as the engine makes it: bang_k_f32_to_f16 into the stretched rows
                big = S.device_buffer(S.LEAD + ix.N * stride + 256)
                held.append(big)
                src, bad = B.DeviceBuffer.from_numpy(ix.vectors()), B.DeviceBuffer(4)
                held += [src, bad]
                ptr = big.ptr + S.LEAD
                _f32_to_f16(B, src.ptr, ptr, ix.N, ix.D, 4 * ix.D, stride, bad.ptr)
                assert int(bad.download(np.uint32, (1,))[0]) == 0
            else:
                big, ptr = S.stretched(ix.graph[:, :vb], stride)
                held.append(big)
            sp.row_layout, sp.d_graph, sp.entry_len, sp.n_rows_hbm, sp.d_rows_hbm = 1, rows.ptr, 256, ix.N, rows.ptr
            sp.rr_vec_base, sp.rr_vec_stride, sp.rr_vec_f16 = ptr, stride, opt.get("f16", 0)
        buf = dict(seed=B.DeviceBuffer.from_numpy(_seed(ix)), q=B.DeviceBuffer.from_numpy(q, slack=16), bloom=B.DeviceBuffer(Q * B.BF_WORDS * 4),
                   cand=B.DeviceBuffer(Q * ROWS * 4), cnt=B.DeviceBuffer(Q * 4), qstats=B.DeviceBuffer(Q * 8), iters=B.DeviceBuffer(Q * 4),
                   ctl=B.DeviceBuffer(64), ids=B.DeviceBuffer(Q * K * 8), dists=B.DeviceBuffer(Q * K * 4))
        held += list(buf.values())
        sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter = Q, ix.R, L, ix.medoid, L + 49
        sp.d_seed, sp.vec_bytes, sp.n_nodes = buf["seed"].ptr, vb, ix.N
        sp.d_bloom, sp.d_cand_ids, sp.d_cand_cnt, sp.d_qstats, sp.d_qiters = buf["bloom"].ptr, buf["cand"].ptr, buf["cnt"].ptr, buf["qstats"].ptr, buf["iters"].ptr
        sp.d_next_query, sp.d_abort = buf["ctl"].ptr, buf["ctl"].ptr + 4
        sp.rr_queries, sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = buf["q"].ptr, B.DTYPE_CODE[ix.dtype], ix.D, K, 0, Q
        sp.rr_ids_out, sp.rr_dists_out = buf["ids"].ptr, buf["dists"].ptr
        if case.entry == "search_exact_beam":
            f = B.lib().bang_k_search_exact_beam
            f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            B._check(f(C.byref(sp), int(case.mode[4]), None), "bang_k_search_exact_beam")
        else:
            B._check(B.lib().bang_k_search_exact(C.byref(sp), None), "bang_k_search_exact")
        B.sync()
        _assert_results(buf["ids"].download(np.uint64, (Q, K)), buf["dists"].download(np.float32, (K, Q)), w)
        _assert_walk(w, buf["iters"].download(np.uint32, (Q,)), buf["cnt"].download(np.uint32, (Q,)), buf["cand"].download(np.uint32, (Q, ROWS)),
                     buf["qstats"].download(np.uint32, (Q, 2)), int(buf["ctl"].download(np.uint32, (2,))[1]))
    finally:
        _free(held)


# ------------------------------------------------------------------------------------------------------------------------ PQ search kernels
def _pq_tables(case, ix):
    """graph entries and code rows at stretched strides in one buffer: -> (buffer, IterState arguments)"""
    se, sc = S.stride_for(case, "graph"), S.stride_for(case, "codes")
    assert sc < 2**32
    big, gptr, cptr = S.stretched_pair(ix.graph, se, ix.codes, sc)
    return big, dict(graph=(gptr, se), codes=(cptr, sc))


@_cases("search", "search_inmem", "search_wf")
def test_query_resident_search_with_fused_rerank(case):
    """bang_k_search, bang_k_search_inmem, bang_k_search_wf: entry_len, code_stride and (the fused re-rank reads the vectors from the graph
    entries) rr_vec_stride stretched together."""
    B = _B()
    ix, q = S.get(case.input)
    w = S.walk(case.input, case.mode)
    fn = B.lib().bang_search_can_rerank
    fn.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32]
    assert fn(B.DTYPE_CODE[ix.dtype], ix.D, S.stride_for(case, "graph"), 0) == 1
    big, tables = _pq_tables(case, ix)
    try:
        extra = 120 if case.entry == "search_inmem" else 50
        st = B.IterState(ix, q, L, ragged=True, extra_iters=extra, **tables)
        assert (st.pq_nhi != 0) == (ix.m in (70, 74))
        iters = st.run_search("bang_k_" + case.entry, rerank_k=K, guard=True)
        _assert_results(st.rr_ids, st.rr_dists, w)
        cnt, log, _ = st.candidates()
        _assert_walk(w, iters, cnt, log, st.d_qstats.download(np.uint32, (Q, 2)), st.abort)
        del st
    finally:
        big.free()


@_cases("search_lut")
def test_lut_search(case):
    """bang_k_search_lut: entry_len and code_stride together; then bang_k_rerank on the same stretched entries."""
    B = _B()
    ix, q = S.get(case.input)
    w = S.walk(case.input, case.mode)
    big, tables = _pq_tables(case, ix)
    try:
        st = B.IterState(ix, q, L, use_lut=True, **tables)
        if not dict(case.opt).get("lut"):
            assert B.pq_layout(ix.chunk_off, ix.D, ix.m)[0] == 0               # a layout that is on the LUT path by itself
        iters = st.run_search_lut()
        cnt, log, _ = st.candidates()
        _assert_walk(w, iters, cnt, log, st.d_qstats.download(np.uint32, (Q, 2)), st.abort)
        _assert_results(*st.rerank(K), w)
        del st
    finally:
        big.free()


@_cases("front_back")
def test_launch_per_iteration_loop(case):
    """bang_k_front + bang_k_back, six iterations on stretched code rows: every iteration's survivors and PQ distances are the reference
    walk's, the candidate log its first entries."""
    B = _B()
    from oracle import oracle as O
    from wordfilter_reference import Reference
    ix, q = S.get(case.input)
    w = S.walk(case.input, case.mode)
    orc, ref = O.Oracle(ix), Reference(ix)
    traces = []
    for i in range(Q):
        traces.append([])
        ref.search_one(q[i], K, L, "split", trace=traces[i])
    big, cptr = S.stretched(ix.codes, S.stride_for(case, "codes"))
    try:
        st = B.IterState(ix, q, L, ragged=True, device_graph=True, codes=(cptr, S.stride_for(case, "codes")))
        for it in range(1, 7):
            st.iter, st.first = it, 1 if it == 1 else 0
            st.run("front")
            cnt, ids, dist = st.nbrs()
            for i in range(Q):
                n, _, s = traces[i][it - 1]
                assert n == it and cnt[i] == len(s) and np.array_equal(ids[i, :cnt[i]], s), (it, i)
                assert np.array_equal(dist[i, :cnt[i]].view(np.uint32), orc.pqdist(orc.lut_build(q[i]), s).view(np.uint32)), (it, i)
            st.run("back")
        ccnt, cids, _ = st.candidates()
        for i in range(Q):
            assert 2 <= ccnt[i] <= 7 and np.array_equal(cids[i, :ccnt[i]], w.logs[i][:ccnt[i]]), i    # (an iteration may go without a parent)
        del st
    finally:
        big.free()


@_cases("pqdist_stream")
def test_pqdist_streaming_form(case):
    """bang_k_pqdist_stream (K2 alone) on stretched code rows."""
    B = _B()
    from oracle import oracle as O
    ix, q = S.get(case.input)
    orc = O.Oracle(ix)
    lists = S.pqdist_lists()
    big, cptr = S.stretched(ix.codes, S.stride_for(case, "codes"))
    try:
        st = B.IterState(ix, q, 16, ragged=True, codes=(cptr, S.stride_for(case, "codes")))
        nb = np.zeros((Q, B.NBR_STRIDE), np.uint32)
        for i, l in enumerate(lists):
            nb[i, :len(l)] = l
        st.d_nbrs.upload(nb)
        st.d_cnt.upload(np.array([len(l) for l in lists], np.uint32))
        st.d_dist.zero()
        p = st.params()
        B._check(B.lib().bang_k_pqdist_stream(C.byref(p), None), "bang_k_pqdist_stream")
        B.sync()
        _, _, dist = st.nbrs()
        for i, l in enumerate(lists):
            assert np.array_equal(dist[i, :len(l)].view(np.uint32), orc.pqdist(orc.lut_build(q[i]), l).view(np.uint32)), i
        del st
    finally:
        big.free()


# ------------------------------------------------------------------------------------------------------------------------ re-rank
def _log_buffers(B, ix, q, w, held):
    ids = np.zeros((Q, ROWS), np.uint32)
    for i, log in enumerate(w.logs):
        ids[i, :len(log)] = log
    b = dict(q=B.DeviceBuffer.from_numpy(q, slack=16), cand=B.DeviceBuffer.from_numpy(ids), cnt=B.DeviceBuffer.from_numpy(np.array([len(x) for x in w.logs], np.uint32)),
             medoid=B.DeviceBuffer.from_numpy(np.ascontiguousarray(ix.graph[ix.medoid]), slack=16), ids=B.DeviceBuffer(Q * K * 8), dists=B.DeviceBuffer(Q * K * 4))
    held += list(b.values())
    return b


def _results(b):
    return b["ids"].download(np.uint64, (Q, K)), b["dists"].download(np.float32, (K, Q))


@_cases("rerank", "rerank_f16")
def test_rerank_from_the_vector_table(case):
    """bang_k_rerank's device-vector form (the grouped 8-bit path, the staged float path, the generic one) and bang_k_rerank_f16: vec_stride
    stretched; the candidate lists are the reference walk's logs."""
    B = _B()
    ix, q = S.get(case.input)
    w = S.walk(case.input, case.mode)
    stride = S.stride_for(case, "vectors")
    held = []
    try:
        b = _log_buffers(B, ix, q, w, held)
        if case.entry == "rerank_f16":
            import fp16_inputs
            table = np.zeros((ix.N, fp16_inputs.row_bytes(ix.D)), np.uint8)
            table[:, :2 * ix.D] = ix.vectors().astype(np.float16).view(np.uint8).reshape(ix.N, 2 * ix.D)
            big, ptr = S.stretched(table, stride)
            held.append(big)
            fn = B.lib().bang_k_rerank_f16
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
            B._check(fn(ptr, stride, b["q"].ptr, b["cand"].ptr, b["cnt"].ptr, ROWS, Q, ix.D, K, 0, b["ids"].ptr, b["dists"].ptr, None), "bang_k_rerank_f16")
        else:
            big, ptr = S.stretched(ix.graph, stride)
            held.append(big)
            fn = B.lib().bang_k_rerank
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
            B._check(fn(ptr, stride, b["medoid"].ptr, b["q"].ptr, B.DTYPE_CODE[ix.dtype], b["cand"].ptr, None, b["cnt"].ptr, ROWS, Q, ix.D, K, 0,
                        b["ids"].ptr, b["dists"].ptr, None), "bang_k_rerank")
        B.sync()
        _assert_results(*_results(b), w)
    finally:
        _free(held)


@pytest.mark.parametrize("form", ["by_row", "by_query"])
@pytest.mark.parametrize("name", ["u8_128_m70", "f32_96_m74"])
def test_rerank_from_a_vector_log(name, form):
    """bang_k_rerank with d_cand_row (vector at (row * Q + q) * vec_stride) and bang_k_rerank_byquery ((q * cand_stride + i) * vec_stride): the
    vec_stride of the log stretched to 16 MiB, the rows / cand_stride such that both products pass 4 and 16 GiB (stretch_inputs.log_slots)."""
    B = _B()
    ix, q = S.get(name)
    w = S.walk(name, "base")
    stride, vb = S.log_stride(ix), ix.D * S.tsize(ix)
    slots = S.log_slots(w.logs, form)
    held = []
    try:
        b = _log_buffers(B, ix, q, w, held)
        big = S.device_buffer(S.LEAD + (int(max(s.max() for s in slots)) + 1) * stride + 256)
        held.append(big)
        for i, log in enumerate(w.logs):
            for c, slot in zip(log[1:], slots[i]):
                big.upload(ix.graph[int(c), :vb], S.LEAD + int(slot) * stride)
        ptr = big.ptr + S.LEAD
        if form == "by_row":
            rows = np.zeros((Q, ROWS), np.uint32)
            for i, log in enumerate(w.logs):
                rows[i, :len(log)] = S.log_rows(len(log))
            d_rows = B.DeviceBuffer.from_numpy(rows)
            held.append(d_rows)
            fn = B.lib().bang_k_rerank
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
            B._check(fn(ptr, stride, b["medoid"].ptr, b["q"].ptr, B.DTYPE_CODE[ix.dtype], b["cand"].ptr, d_rows.ptr, b["cnt"].ptr, ROWS, Q, ix.D, K, 0,
                        b["ids"].ptr, b["dists"].ptr, None), "bang_k_rerank")
        else:
            fn = B.lib().bang_k_rerank_byquery
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p] * 3
            B._check(fn(ptr, stride, b["medoid"].ptr, b["q"].ptr, B.DTYPE_CODE[ix.dtype], b["cand"].ptr, b["cnt"].ptr, ROWS, 0, Q, Q, ix.D, K, 0,
                        b["ids"].ptr, b["dists"].ptr, None), "bang_k_rerank_byquery")
        B.sync()
        _assert_results(*_results(b), w)
    finally:
        _free(held)


# ------------------------------------------------------------------------------------------------------------------------ fp16 conversion
@pytest.mark.parametrize("D", S.CONVERT_D)
def test_f32_to_f16_conversion(D, convert):  # noqa: F811
    """bang_k_f32_to_f16: 640 rows, src_stride and dst_stride both stretched (one buffer), against csrc/bang_f16.h compiled for the host."""
    B = _B()
    import fp16_inputs
    src = S.convert_rows(D)
    rb = fp16_inputs.row_bytes(D)
    ss, ds = S.stride_of(4 * D), S.stride_of(rb)
    want, over = convert(src.view(np.uint32).reshape(-1))
    assert not over.any()
    big, sptr, dptr = S.stretched_pair(src, ss, np.full((S.N, rb), 0xAB, np.uint8), ds)
    bad = B.DeviceBuffer(4)
    try:
        _f32_to_f16(B, sptr, dptr, S.N, D, ss, ds, bad.ptr)
        assert int(bad.download(np.uint32, (1,))[0]) == 0
        got = np.empty((S.N, rb), np.uint8)
        for i in range(S.N):
            B._check(B.lib().bang_dev_d2h(C.c_void_p(got[i].ctypes.data), C.c_void_p(dptr + i * ds), C.c_size_t(rb)), "bang_dev_d2h")
        assert np.array_equal(got[:, :2 * D].copy().view(np.uint16).reshape(S.N, D), want.reshape(S.N, D))
        assert not got[:, 2 * D:].any()                                        # the padding half of an odd row
    finally:
        big.free()
        bad.free()


# ------------------------------------------------------------------------------------------------------------------------ engine level
@_cases("engine")
def test_engine_hands_the_code_stride_on(case):
    """Engine.load_index with the caller's stretched code table (d_codes, code_stride): how bang_alloc and bang_lane pass the stride on, one
    case per engine option set."""
    import bang_amd
    B = _B()
    ix, q = S.get(case.input)
    w = S.walk(case.input, case.mode)
    opt = dict(case.opt)
    opt.setdefault("graph", bang_amd.GRAPH_DEVICE)
    stride = S.stride_for(case, "codes")
    big, cptr = S.stretched(ix.codes, stride)
    try:
        with bang_amd.Engine(ix.dtype, **opt) as e:
            e.load_index(ix, d_codes=cptr, code_stride=stride)
            e.set_searchparams(K, L)
            e.alloc(Q)
            e.init(Q)
            ids, d = e.query(q)
            s = e.stats()
            assert s["search_kernel"] == 1 and s["code_stride"] == stride, s
            st = e.query_counters(Q)
            log, cnt = e.candidate_log(Q, L, 120 if opt.get("semantics") else 50)
            e.free()
            e.unload()
        _assert_results(ids, d, w)
        assert np.array_equal(st, w.stats)
        for i in range(Q):
            assert np.array_equal(log[i, :cnt[i]], w.logs[i]), i
    finally:
        big.free()
