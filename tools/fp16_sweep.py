#!/usr/bin/env python3
"""The HBM vector table of a float index as fp32 against fp16 (option vectors_fp16), graph = host with the adjacency rows pulled (pull = 1).

Builds a DEEP-like structured synthetic index (tools/exact_sweep.py's builder and cache; D = 96, m = 74) and measures, per table:

  re-rank launch   bang_k_rerank on the float table / bang_k_rerank_f16 on the fp16 table (built by bang_k_f32_to_f16), alone, on the candidate
                   log of one PQ batch at --rerank-L: --launches launches back to back behind one warm-up, one synchronisation, mean per launch
  pq-pull          whole-batch queries/s of the pulled PQ walk (distance = 0): fp32 table with the re-rank fused into the search launch (the
                   default), fp32 table with the re-rank as a launch of its own (fuse_rerank = 0) and fp16 table (always a launch of its own)
  exact-pull       distance = 1 on either table, and the smallest L of the sweep at which 10-recall@10 >= --target

Per configuration and L: one warm-up bang_query and --runs timed ones on the whole batch (bang_init outside the timed region), best and median,
10-recall@10 against the ground truth of the ORIGINAL vectors.  Every row carries what bang_get_stats reports (vectors_fp16, vector_table_bytes,
rerank_fused).

  python tools/fp16_sweep.py --workload deep200k --out fp16_deep200k.json

Not part of bench.py: the measurement behind profiles/vectors_fp16.md.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bang_amd  # noqa: E402
from bang_amd import binding as B  # noqa: E402
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402

exact_sweep.WORKLOADS.update({"deep200k": (200_000, 96, "float", 64, 74, 128)})
DIST = {"pq": bang_amd.DISTANCE_PQ, "exact": bang_amd.DISTANCE_EXACT}


def measure(e, name, mode, q, gi, gd, Ls, k, runs, log):
    rows = []
    Q = q.shape[0]
    e.set_option("distance", DIST[mode])
    for L in Ls:
        e.set_searchparams(k, L)
        e.alloc(Q)
        times, ids = [], None
        for r in range(runs + 1):                             # run 0: warm-up
            e.init(Q)
            t0 = time.perf_counter()
            ids, _ = e.query(q)
            dt = time.perf_counter() - t0
            if r:
                times.append(dt)
        st = e.query_counters(Q)
        s = e.stats()
        e.free()
        row = {"config": name, "mode": mode, "L": L, "recall": round(O.recall(gi, gd, ids, k), 3), "qps_best": round(Q / min(times)),
               "qps_median": round(Q / float(np.median(times))), "ms_best": round(1e3 * min(times), 3), "ms_median": round(1e3 * float(np.median(times)), 3),
               "evals": round(float(st[:, 2].mean()), 1), "expanded": round(float(st[:, 1].mean()), 2), "vectors_fp16": int(s["vectors_fp16"]),
               "vector_table_bytes": int(s["vector_table_bytes"]), "rerank_fused": int(s["rerank_fused"]), "graph_pull": int(s["graph_pull"])}
        log(json.dumps(row))
        rows.append(row)
    return rows


def rerank_alone(ix, q, L, k, launches, log):
    """The two re-rank launches alone on one candidate log (the PQ walk's, fp32 table, at this L)."""
    Q = q.shape[0]
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0) as e:
        e.load_index(ix)
        e.set_searchparams(k, L)
        e.alloc(Q)
        e.init(Q)
        e.query(q)
        cand, cnt = e.candidate_log(Q, L)
        e.free()
        e.unload()
    lib = B.lib()
    row = (2 * ix.D + 3) & ~3
    vec = ix.vectors()
    d_f32 = B.DeviceBuffer.from_numpy(vec, slack=256)
    d_f16 = B.DeviceBuffer(ix.N * row + 256)
    conv = lib.bang_k_f32_to_f16
    conv.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    B._check(conv(d_f32.ptr, d_f16.ptr, ix.N, ix.D, 4 * ix.D, row, None, None), "bang_k_f32_to_f16")
    d_q = B.DeviceBuffer.from_numpy(np.ascontiguousarray(q, np.float32), slack=16)
    d_cand, d_cnt = B.DeviceBuffer.from_numpy(cand), B.DeviceBuffer.from_numpy(cnt)
    d_ids, d_d = B.DeviceBuffer(Q * k * 8), B.DeviceBuffer(Q * k * 4)
    d_med = B.DeviceBuffer.from_numpy(vec[ix.medoid], slack=16)
    f32 = lib.bang_k_rerank
    f32.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
    f16 = lib.bang_k_rerank_f16
    f16.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 3
    calls = {"fp32": lambda: f32(d_f32.ptr, 4 * ix.D, d_med.ptr, d_q.ptr, B.F32, d_cand.ptr, None, d_cnt.ptr, cand.shape[1], Q, ix.D, k, 0, d_ids.ptr, d_d.ptr, None),
             "fp16": lambda: f16(d_f16.ptr, row, d_q.ptr, d_cand.ptr, d_cnt.ptr, cand.shape[1], Q, ix.D, k, 0, d_ids.ptr, d_d.ptr, None)}
    out = {"L": L, "Q": Q, "candidates_per_query": round(float(cnt.mean()), 1), "launches": launches}
    for rep in range(3):                                      # the two interleaved, three times
        for name, call in calls.items():
            B._check(call(), name)
            B.sync()
            t0 = time.perf_counter()
            for _ in range(launches):
                B._check(call(), name)
            B.sync()
            out.setdefault(name + "_us", []).append(round(1e6 * (time.perf_counter() - t0) / launches, 1))
    log(json.dumps({"rerank_alone": out}))
    for b in (d_f32, d_f16, d_q, d_cand, d_cnt, d_ids, d_d, d_med):
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="deep200k", choices=sorted(exact_sweep.WORKLOADS))
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=82)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--rerank-L", type=int, default=46)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--target", type=float, default=90.0)
    ap.add_argument("--cache", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    ix, q, gi, gd = exact_sweep.workload(a.workload, a.queries, a.cache, log)
    if ix.dtype != "float":
        raise SystemExit("vectors_fp16 applies to float indexes")
    out = {"workload": a.workload, "N": int(ix.N), "D": int(ix.D), "m": int(ix.m), "R": int(ix.R), "Q": int(q.shape[0]), "k": k, "runs": a.runs,
           "rows": [], "at_target": {}}
    out["rerank_alone"] = rerank_alone(ix, q, a.rerank_L, k, a.launches, log)
    configs = (("fp32-fused", dict(vectors_fp16=0)), ("fp32-launch", dict(vectors_fp16=0, fuse_rerank=0)), ("fp16", dict(vectors_fp16=1)))
    for name, opts in configs:
        with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0, **opts) as e:
            e.load_index(ix)
            out["rows"] += measure(e, f"pq-pull-{name}", "pq", q, gi, gd, Ls, k, a.runs, log)
            if name != "fp32-launch" and ix.D % 8 == 0 and ix.D <= 256:
                out["rows"] += measure(e, f"exact-pull-{name.split('-')[0]}", "exact", q, gi, gd, Ls, k, a.runs, log)
            e.unload()
    for name in sorted({r["config"] for r in out["rows"]}):
        hit = [r for r in out["rows"] if r["config"] == name and r["recall"] >= a.target]
        out["at_target"][name] = hit[0] if hit else None
        log(f"{name}: smallest L with recall >= {a.target}: " + (f"L = {hit[0]['L']}, {hit[0]['qps_best']} queries/s" if hit else "none in the sweep"))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
