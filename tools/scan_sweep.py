"""The exact scan against what it replaces: python tools/scan_sweep.py [--workloads sift1m,deep1m] [--out profiles/scan.md]

One process, one GPU, the structured 10^6-point indexes of tools/exact_sweep.py (uint8 m = 32, float m = 74).  Per workload, the contenders run
alternately, one warm-up and five timed runs each, medians recorded:

  * Engine.scan for Q = 100 and 10 000 at k = 10 and 100, split into scan launches and merge (Engine.scan_times)
  * the same truth by bang_amd.synth.knn on the same GPU -- what the tools use today -- and how many of its ids differ from the scan's, tie-aware
    (an id of the scan's answer is missed when synth.knn neither lists it nor lists the scan's k-th distance in its place)
  * the exact-distance walk at the smallest L of the list that reaches 90 % 10-recall@10 against the scan
  * label shares 50 / 10 / 1 % (tools/labels_sweep.py's table): the scan's time beside the filtered walk's time and its recall against the scan
  * the 8-bit kernel's share of the i8 MFMA rate: 2 N Q D operations over the scan launches' time, against 2 x the dense BF16 rate of the chip

--any [--out profiles/scan_any.md]: the layouts of option scan_any instead, through the kernel entry bang_k_scan_any on a packed table of 10^6
structured vectors (synth.make_vectors / make_queries; no graph is built, so no engine is loaded: the times are the launches' -- scan, merge, outputs --
without the engine's copies of queries and results), against synth.knn on the same GPU; and uint8 D = 256 on scan8_any_kernel beside scan8_kernel.

--mfma [--out profiles/scan_mfma.md]: option scan_mfma's kernel entry bang_k_scan_f32_mfma beside the float chain kernel (bang_k_scan_any) and synth.knn
on float D = 74, 201 (MIPS) and 960, the three alternating, with the share of the tested pairs that the exact refine took.

--radix [--out profiles/scan_radix.md]: option scan_radix's kernel entry bang_k_scan_radix on packed tables of uint8 D = 128, float D = 96 and int8
D = 100: at k = 10 / 100 beside the entry the scan takes today (bang_k_scan, bang_k_scan_any for D = 100), at k = 1000 / 4096 beside synth.knn, with
the digit passes a launch needed and the share of its queries that went on into id digits (read from the launch's scratch).
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bang_amd  # noqa: E402
from bang_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402
import labels_sweep  # noqa: E402

RUNS = 5
I8_PEAK_OPS = 2 * 2.5e15            # i8 MFMA = 2 x the dense BF16 rate (MI355X: 2.5 PFLOP/s BF16)
SHARES = (50, 10, 1)
WALK_LS = (10, 14, 20, 28, 40, 56, 80, 112, 160)


def median_ms(fn, runs=RUNS):
    fn()                                                  # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def alternate_ms(fns, runs=RUNS):
    """the contenders in turn, run after run: one warm-up each, then the median of `runs` per contender"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(t)) for t in ts]


def missed(scan_ids, scan_d, knn_ids):
    """ids of the scan's answer that synth.knn does not return, tie-aware: an id at the scan's k-th distance may be swapped for another at that distance"""
    bad = 0
    for i in range(scan_ids.shape[0]):
        absent = ~np.isin(scan_ids[i].astype(np.int64), knn_ids[i].astype(np.int64))
        bad += int((absent & (scan_d[:, i] != scan_d[-1, i])).sum())
    return bad


def walk(e, q, k, L):
    Q = q.shape[0]
    e.set_searchparams(k, L)
    e.alloc(Q)
    out = {}

    def run():
        e.init(Q)
        out["ids"] = e.query(q)[0]
    ms = median_ms(run)
    e.free()
    return ms, out["ids"]


def one(name, log):
    import torch
    rows = []
    ix, q_all, _, _ = exact_sweep.workload(name, 10000, None, log)
    N, D = int(ix.N), int(ix.D)
    dev_vec = torch.from_numpy(ix.vectors()).cuda()
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT) as e:
        e.load_index(ix)
        for Q in (100, 10000):
            q = np.ascontiguousarray(q_all[:Q])
            dev_q = torch.from_numpy(q).cuda()
            for k in (10, 100):
                res = {}

                def scan():
                    res["scan"] = e.scan(q, k)
                    res["t"] = e.scan_times()

                def knn():
                    i, d = synth.knn(dev_vec, dev_q, k)
                    res["knn"] = i.cpu().numpy()
                ms_scan, ms_knn = alternate_ms([scan, knn])
                ids, d, _ = res["scan"]
                row = dict(workload=name, Q=Q, k=k, scan_ms=round(ms_scan, 3), scan_launch_ms=round(res["t"]["scan"], 3), merge_ms=round(res["t"]["merge"], 3),
                           knn_ms=round(ms_knn, 3), knn_ids_missed=missed(ids, d, res["knn"]), results=Q * k)
                if ix.dtype != "float":
                    row["i8_mfma_share"] = round(2.0 * N * Q * D / (res["t"]["scan"] * 1e-3) / I8_PEAK_OPS, 4)
                log(json.dumps(row))
                rows.append(row)
        # the exact-distance walk at the smallest L reaching 90 % against the scan, Q = 10 000, k = 10
        q = np.ascontiguousarray(q_all[:10000])
        truth = e.scan(q, 10)
        gt_i, gt_d = (truth[0] & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(truth[1].T)
        for L in WALK_LS:
            ms, ids = walk(e, q, 10, L)
            rec = O.recall(gt_i, gt_d, ids, 10)
            if rec >= 90.0 or L == WALK_LS[-1]:
                row = dict(workload=name, Q=10000, k=10, walk_L=L, walk_ms=round(ms, 3), walk_recall=round(rec, 2))
                log(json.dumps(row))
                rows.append(row)
                break
        # label shares: the scan beside the filtered walk at L = 94, Q = 1 000
        q = np.ascontiguousarray(q_all[:1000])
        labels = labels_sweep.label_table(N, SHARES)
        e.set_labels(labels)
        for b, s in enumerate(SHARES):
            filt = (np.full(1000, 1 << b, np.uint32), np.zeros(1000, np.uint32))
            res = {}

            def scan_f():
                res["scan"] = e.scan(q, 10, *filt)
            e.set_searchparams(10, 94)
            e.alloc(1000)
            e.set_filters(*filt)

            def walk_f():
                e.init(1000)
                res["walk"] = e.query(q)[0]
            ms_scan, ms_walk = alternate_ms([scan_f, walk_f])
            e.free()
            ids, d, matched = res["scan"]
            wids = res["walk"]
            rec = O.recall((ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(d.T), wids, 10)
            row = dict(workload=name, Q=1000, k=10, share=s, scan_ms=round(ms_scan, 3), matched_mean=round(float(matched.mean()), 1), walk_L=94,
                       walk_ms=round(ms_walk, 3), walk_recall_vs_scan=round(rec, 2))
            log(json.dumps(row))
            rows.append(row)
        e.unload()
    return rows


ANY_LAYOUTS = (("u8_784", 784, "uint8", 0), ("i8_100", 100, "int8", 0), ("f32_960", 960, "float", 0), ("f32_201_mips", 201, "float", 1))


def k_scan(entry, vec, stride, dtype, D, q, qdim, k):
    """one launch of bang_k_scan / bang_k_scan_any on device tensors -> a function that runs it and waits, and its outputs (ids [Q][k], dists [k][Q])"""
    import ctypes as C
    import torch
    from bang_amd import binding as B
    lib, Q, N = B.lib(), q.shape[0], vec.shape[0]
    mfma, radix = entry == "bang_k_scan_f32_mfma", entry == "bang_k_scan_radix"
    lib.bang_scan_radix_geometry.argtypes = [C.c_int] + [C.c_uint32] * 4 + [C.c_void_p] * 3
    lib.bang_scan_radix_scratch_bytes.argtypes, lib.bang_scan_radix_scratch_bytes.restype = [C.c_uint32] * 3, C.c_uint64
    lib.bang_scan_any_geometry.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.bang_scan_f32_mfma_geometry.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.bang_scan_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.bang_scan_scratch_bytes.restype = C.c_uint64
    t, st = C.c_uint32(0), C.c_uint32(0)
    if radix:
        assert lib.bang_scan_radix_geometry(B.DTYPE_CODE[dtype], D, Q, N, k, C.byref(t), C.byref(st), None) == 0
    elif mfma:
        assert lib.bang_scan_f32_mfma_geometry(D, Q, N, k, C.byref(t), C.byref(st)) == 0
    else:
        assert lib.bang_scan_any_geometry(B.DTYPE_CODE[dtype], D, Q, N, k, C.byref(t), C.byref(st)) == 0
    nbytes = int((lib.bang_scan_radix_scratch_bytes if radix else lib.bang_scan_scratch_bytes)(Q, k, st.value))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    ids, dists = torch.empty((Q, k), dtype=torch.int64, device="cuda"), torch.empty((k, Q), dtype=torch.float32, device="cuda")
    matched = torch.empty(Q, dtype=torch.int32, device="cuda")
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")          # bang_k_scan_f32_mfma: pairs tested, pairs refined
    p = B.ScanParams()
    p.d_vec_base, p.vec_stride, p.dtype, p.D, p.n_nodes = vec.data_ptr(), stride, B.DTYPE_CODE[dtype], D, N
    p.d_queries, p.nq, p.k, p.stripes = q.data_ptr(), Q, k, st.value
    p.d_scratch, p.scratch_bytes, p.d_ids_out, p.d_dists_out, p.d_matched = scratch.data_ptr(), nbytes, ids.data_ptr(), dists.data_ptr(), matched.data_ptr()
    fn = getattr(lib, entry)
    with_qdim = entry in ("bang_k_scan_any", "bang_k_scan_radix")
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p] if with_qdim else [C.c_void_p, C.c_void_p]
    args = (C.byref(p), qdim, None) if with_qdim else (C.byref(p), None)
    if mfma:
        fn.argtypes, args = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], (C.byref(p), qdim, C.c_void_p(counters.data_ptr()), None)

    def run():
        assert fn(*args) == 0, lib.bang_last_error().decode()
        torch.cuda.synchronize()
    return run, (ids, dists), (p, scratch, matched, counters)


def any_rows(log):
    import torch
    rows = []
    for name, D, dtype, drop in ANY_LAYOUTS:
        x = synth.make_vectors(1_000_000, D, dtype, n_clusters=256, seed=77, device="cuda")
        q_all = synth.make_queries(x, 10000, dtype, seed=77)
        vec = x.contiguous() if dtype == "float" else x.to(torch.uint8 if dtype == "uint8" else torch.int8).contiguous()
        for Q in (100, 10000):
            qk = q_all[:Q].clone()
            if drop:
                qk[:, D - 1] = 0                          # the MIPS coordinate: synth.knn sees the 0 the scan reads
            q = (qk if dtype == "float" else qk.to(vec.dtype))[:, :D - drop].contiguous()
            for k in (10, 100):
                run, out, keep = k_scan("bang_k_scan_any", vec, vec.shape[1] * vec.element_size(), dtype, D, q, D - drop, k)
                res = {}

                def knn():
                    res["knn"] = synth.knn(x, qk, k)[0].cpu().numpy()
                ms_scan, ms_knn = alternate_ms([run, knn])
                ids, d = out[0].cpu().numpy().astype(np.uint64), out[1].cpu().numpy()
                row = dict(workload=name, Q=Q, k=k, scan_ms=round(ms_scan, 3), knn_ms=round(ms_knn, 3), knn_ids_missed=missed(ids, d, res["knn"]), results=Q * k)
                if dtype != "float":
                    row["i8_mfma_share"] = round(2.0 * 1e6 * Q * D / (ms_scan * 1e-3) / I8_PEAK_OPS, 4)
                log(json.dumps(row))
                rows.append(row)
        del x, vec, q_all
        torch.cuda.empty_cache()
    # the price of queries in LDS and a runtime KS: uint8 D = 256 and D = 1024 (the share of the MFMA rate at the widest layout)
    for D in (256, 1024):
        x = synth.make_vectors(1_000_000, D, "uint8", n_clusters=256, seed=78, device="cuda")
        vec = x.to(torch.uint8).contiguous()
        q = synth.make_queries(x, 10000, "uint8", seed=78).to(torch.uint8).contiguous()
        runs = [k_scan("bang_k_scan_any", vec, D, "uint8", D, q, D, 10)]
        if D == 256:
            runs.append(k_scan("bang_k_scan", vec, D, "uint8", D, q, D, 10))
        ms = alternate_ms([r[0] for r in runs])
        same = len(runs) == 1 or bool(torch.equal(runs[0][1][0], runs[1][1][0]) and torch.equal(runs[0][1][1], runs[1][1][1]))
        row = dict(workload=f"u8_{D}", Q=10000, k=10, any_ms=round(ms[0], 3), narrow_ms=round(ms[1], 3) if len(ms) > 1 else None, same_bits=same,
                   i8_mfma_share=round(2.0 * 1e6 * 10000 * D / (ms[0] * 1e-3) / I8_PEAK_OPS, 4))
        log(json.dumps(row))
        rows.append(row)
        del x, vec, q, runs
        torch.cuda.empty_cache()
    return rows


RADIX_LAYOUTS = (("u8_128", 128, "uint8", "bang_k_scan"), ("f32_96", 96, "float", "bang_k_scan"), ("i8_100", 100, "int8", "bang_k_scan_any"))


def radix_rows(log):
    """bang_k_scan_radix beside today's entry (k <= 128) and beside synth.knn (k > 128)"""
    import torch
    rows = []
    for name, D, dtype, today in RADIX_LAYOUTS:
        x = synth.make_vectors(1_000_000, D, dtype, n_clusters=256, seed=77, device="cuda")
        q_all = synth.make_queries(x, 10000, dtype, seed=77)
        vec = x.contiguous() if dtype == "float" else x.to(torch.uint8 if dtype == "uint8" else torch.int8).contiguous()
        stride = vec.shape[1] * vec.element_size()
        for Q in (100, 10000):
            qk = q_all[:Q].clone()
            q = (qk if dtype == "float" else qk.to(vec.dtype)).contiguous()
            for k in (10, 100, 1000, 4096):
                run, out, keep = k_scan("bang_k_scan_radix", vec, stride, dtype, D, q, D, k)
                res = {}
                if k <= 128:
                    other, out_o, keep_o = k_scan(today, vec, stride, dtype, D, q, D, k)
                else:
                    def other():
                        res["knn"] = synth.knn(x, qk, k)[0].cpu().numpy()
                ms_radix, ms_other = alternate_ms([run, other])
                fixed = keep[1].view(torch.int32)[(2 + 256 + 1) * Q:(2 + 256 + 2) * Q].cpu().numpy()     # the scratch layout: bang_scan_radix_scratch_bytes
                skipped = 4 - (int(vec.shape[0] - 1).bit_length() + 7) // 8     # id digits above the width of N - 1: never launched
                digits = int(fixed.max()) // 8                             # the lowest digit any query of the launch still needed
                row = dict(workload=name, Q=Q, k=k, radix_ms=round(ms_radix, 3), passes=digits - (skipped if digits > 4 else 0), id_digit_share=round(float((fixed > 32).mean()), 5),
                           runs=int(keep[0].stripes))
                if k <= 128:
                    row.update(today=today, today_ms=round(ms_other, 3),
                               same_bits=bool(torch.equal(out[0], out_o[0]) and torch.equal(out[1].view(torch.int32), out_o[1].view(torch.int32))))
                    del other, out_o, keep_o
                else:
                    ids, d = out[0].cpu().numpy().astype(np.uint64), out[1].cpu().numpy()
                    row.update(knn_ms=round(ms_other, 3), knn_ids_missed=missed(ids, d, res["knn"]), results=Q * k)
                log(json.dumps(row))
                rows.append(row)
                del run, out, keep
                torch.cuda.empty_cache()
        del x, vec, q_all
        torch.cuda.empty_cache()
    return rows


def markdown_radix(rows, commit):
    out = ["# Exact scan, option scan_radix (tools/scan_sweep.py --radix)", "",
           f"Commit {commit}, {datetime.date.today().isoformat()}, one MI355X, one process, the two contenders alternated, one warm-up and the median of {RUNS} runs.  "
           "10^6 structured vectors in a packed table, through the kernel entries: host wall time in ms of the launches up to their completion, queries "
           "and results staying on the device.  passes: the histogram + pick passes that still had an unresolved query (of the 4 distance digits and the "
           "3 id digits 10^6 points need); id digits: the share of the queries whose rank-k distance was tied beyond the cut.", "",
           "## k <= 128: beside the entry the scan takes today", "",
           "| layout | Q | k | radix ms | today ms | today's entry | same bits | passes | id digits | runs |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "today_ms" in r:
            out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['radix_ms']} | {r['today_ms']} | {r['today']} | {r['same_bits']} | {r['passes']} | "
                       f"{r['id_digit_share']} | {r['runs']} |")
    out += ["", "## k > 128: beside synth.knn on the same GPU", "",
            "| layout | Q | k | radix ms | synth.knn ms | knn ids missed (tie-aware) | passes | id digits | runs |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "knn_ms" in r:
            out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['radix_ms']} | {r['knn_ms']} | {r['knn_ids_missed']} of {r['results']} | {r['passes']} | "
                       f"{r['id_digit_share']} | {r['runs']} |")
    return "\n".join(out) + "\n"


MFMA_LAYOUTS = (("f32_74", 74, 0), ("f32_201_mips", 201, 1), ("f32_960", 960, 0))


def mfma_rows(log):
    import torch
    rows = []
    for name, D, drop in MFMA_LAYOUTS:
        x = synth.make_vectors(1_000_000, D, "float", n_clusters=256, seed=77, device="cuda").contiguous()
        q_all = synth.make_queries(x, 10000, "float", seed=77)
        for Q in (100, 10000):
            qk = q_all[:Q].clone()
            if drop:
                qk[:, D - 1] = 0                          # the MIPS coordinate: synth.knn sees the 0 the scan reads
            q = qk[:, :D - drop].contiguous()
            for k in (10, 100):
                chain, out_c, keep_c = k_scan("bang_k_scan_any", x, 4 * D, "float", D, q, D - drop, k)
                mfma, out_m, keep_m = k_scan("bang_k_scan_f32_mfma", x, 4 * D, "float", D, q, D - drop, k)
                res = {}

                def knn():
                    res["knn"] = synth.knn(x, qk, k)[0].cpu().numpy()
                ms_chain, ms_mfma, ms_knn = alternate_ms([chain, mfma, knn])
                tested, refined = (int(v) for v in keep_m[3].cpu())
                row = dict(workload=name, Q=Q, k=k, chain_ms=round(ms_chain, 3), mfma_ms=round(ms_mfma, 3), knn_ms=round(ms_knn, 3),
                           same_bits=bool(torch.equal(out_c[0], out_m[0]) and torch.equal(out_c[1].view(torch.int32), out_m[1].view(torch.int32))),
                           tested=tested, refined_share=round(refined / max(tested, 1), 5), stripes=int(keep_m[0].stripes))
                log(json.dumps(row))
                rows.append(row)
                del chain, mfma, out_c, out_m, keep_c, keep_m
        del x, q_all
        torch.cuda.empty_cache()
    return rows


def markdown_mfma(rows, commit):
    out = ["# Exact scan, option scan_mfma (tools/scan_sweep.py --mfma)", "",
           f"Commit {commit}, {datetime.date.today().isoformat()}, one MI355X, one process, the three contenders alternated, one warm-up and the median of {RUNS} runs.  "
           "10^6 structured float vectors in a packed table, through the kernel entries: host wall time in ms of the launches (scan, merge, outputs) up to "
           "their completion, queries and results staying on the device.  chain: bang_k_scan_any (scan_f32_any_kernel); mfma: bang_k_scan_f32_mfma; "
           "refined share: pairs the exact chain ran for over pairs tested.", "",
           "| layout | Q | k | chain ms | mfma ms | synth.knn ms | same bits | refined share | stripes (mfma) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['chain_ms']} | {r['mfma_ms']} | {r['knn_ms']} | {r['same_bits']} | {r['refined_share']} | {r['stripes']} |")
    return "\n".join(out) + "\n"


def markdown_any(rows, commit):
    out = ["# Exact scan, option scan_any (tools/scan_sweep.py --any)", "",
           f"Commit {commit}, {datetime.date.today().isoformat()}, one MI355X, one process, contenders alternated, one warm-up and the median of {RUNS} runs.  "
           "10^6 structured vectors in a packed table, through bang_k_scan_any: host wall time in ms of the launches (scan, merge, outputs) up to their "
           "completion, queries and results staying on the device.", "",
           "| layout | Q | k | scan ms | synth.knn ms | knn ids missed (tie-aware) | share of the i8 MFMA rate |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        if "knn_ms" in r:
            out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['scan_ms']} | {r['knn_ms']} | {r['knn_ids_missed']} of {r['results']} | {r.get('i8_mfma_share', '-')} |")
    out += ["", "## scan8_any_kernel beside scan8_kernel (uint8, Q = 10 000, k = 10)", "",
            "| layout | scan8_any_kernel ms | scan8_kernel ms | same bits | share of the i8 MFMA rate (any) |", "|---|---|---|---|---|"]
    for r in rows:
        if "any_ms" in r:
            out.append(f"| {r['workload']} | {r['any_ms']} | {r['narrow_ms'] if r['narrow_ms'] is not None else '-'} | {r['same_bits']} | {r['i8_mfma_share']} |")
    return "\n".join(out) + "\n"


def markdown(rows, commit):
    out = [f"# Exact scan (tools/scan_sweep.py)", "",
           f"Commit {commit}, {datetime.date.today().isoformat()}, one MI355X, one process, contenders alternated, one warm-up and the median of {RUNS} runs.  "
           "Times are host wall time of the whole call in ms (scan launches / merge: GPU time between events).", "",
           "## Scan against synth.knn", "",
           "| workload | Q | k | scan ms | scan launches ms | merge ms | synth.knn ms | knn ids missed (tie-aware) | share of the i8 MFMA rate |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "knn_ms" in r:
            out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['scan_ms']} | {r['scan_launch_ms']} | {r['merge_ms']} | {r['knn_ms']} | "
                       f"{r['knn_ids_missed']} of {r['results']} | {r.get('i8_mfma_share', '-')} |")
    out += ["", "## The exact-distance walk at the smallest L reaching 90 % 10-recall@10 against the scan (Q = 10 000)", "",
            "| workload | L | walk ms | recall % |", "|---|---|---|---|"]
    for r in rows:
        if "walk_recall" in r:
            out.append(f"| {r['workload']} | {r['walk_L']} | {r['walk_ms']} | {r['walk_recall']} |")
    out += ["", "## Label filters (Q = 1 000, k = 10): the scan beside the filtered walk at L = 94", "",
            "| workload | share % | matched (mean) | scan ms | walk ms | walk recall against the scan % |", "|---|---|---|---|---|---|"]
    for r in rows:
        if "share" in r:
            out.append(f"| {r['workload']} | {r['share']} | {r['matched_mean']} | {r['scan_ms']} | {r['walk_ms']} | {r['walk_recall_vs_scan']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--any", action="store_true", help="the layouts of option scan_any, through the kernel entry (default --out: profiles/scan_any.md)")
    ap.add_argument("--mfma", action="store_true", help="option scan_mfma's kernel entry beside the float chain kernel and synth.knn (default --out: profiles/scan_mfma.md)")
    ap.add_argument("--radix", action="store_true", help="option scan_radix's kernel entry beside today's entries and synth.knn (default --out: profiles/scan_radix.md)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tables are headed with (default: git rev-parse of this tree)")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)      # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("scan_sweep needs a HIP device")
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "(no git)"
    except OSError:
        commit = "(no git)"
    a.out = a.out or os.path.join(ROOT, "profiles", "scan_radix.md" if a.radix else "scan_mfma.md" if a.mfma else "scan_any.md" if a.any else "scan.md")
    if a.any or a.mfma or a.radix:
        rows = radix_rows(log) if a.radix else mfma_rows(log) if a.mfma else any_rows(log)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        with open(a.out, "w") as f:
            f.write((markdown_radix if a.radix else markdown_mfma if a.mfma else markdown_any)(rows, commit))
        log(f"wrote {a.out}")
        return
    rows = []
    for name in a.workloads.split(","):                   # the files are rewritten behind every workload: a run cut short keeps what it has
        rows += one(name, log)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        with open(a.out, "w") as f:
            f.write(markdown(rows, commit))
    log(f"wrote {a.out}")


if __name__ == "__main__":
    main()
