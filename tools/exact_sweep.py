#!/usr/bin/env python3
"""PQ walk + re-rank (distance = 0) against exact distances in the walk (distance = 1) over an L sweep, graph in HBM.

Builds a structured synthetic index (bang_amd.synth: kNN + random-link graph, trained PQ, brute-force ground truth), then for each mode and
each L of the harness grid (L = k, k + 12, ..., test_driver.cpp) runs the engine on the whole query batch: one warm-up run and --runs timed
bang_query calls (bang_init outside the timed region, as the harness does).  Reports per mode and L: 10-recall@10, QPS (best and median of the
timed runs), mean iterations and distance evaluations per query; then per mode the smallest L with recall >= --target and its QPS.

  python tools/exact_sweep.py --workload sift1m --out exact_sift1m.json
  python tools/exact_sweep.py --workload deep1m --cache ~/exact_cache/deep1m --modes exact --Ls 46 --runs 1     (one launch, e.g. under rocprofv3)

Not part of bench.py: the measurement behind profiles/exact_distance.md.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))

import bang_amd  # noqa: E402
from bang_amd import formats, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

# name: (N, D, dtype, R, m, clusters)
WORKLOADS = {
    "sift1m": (1_000_000, 128, "uint8", 64, 32, 256),     # SIFT1M-like (bench.py's sift1m workload)
    "deep1m": (1_000_000, 96, "float", 64, 74, 256),      # DEEP-like layout (D = 96, m = 74) at the largest N synth builds by brute force
    "small": (100_000, 128, "uint8", 64, 32, 64),
}
MODES = {"pq": bang_amd.DISTANCE_PQ, "exact": bang_amd.DISTANCE_EXACT}


def workload(name, Q, cache, log):
    N, D, dtype, R, m, ncl = WORKLOADS[name]
    if cache and os.path.exists(cache + "_queries.npy"):
        ix = formats.read_index(cache, dtype)
        return ix, np.load(cache + "_queries.npy"), np.load(cache + "_gt_ids.npy"), np.load(cache + "_gt_dists.npy")
    t0 = time.time()
    dev = "cuda" if bang_amd.device_count() > 0 else "cpu"
    ix, q, gi, gd = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=ncl, device=dev)
    log(f"built {name}: N={N} D={D} {dtype} R={R} m={m} Q={Q} in {time.time() - t0:.1f} s")
    if cache:
        os.makedirs(os.path.dirname(cache) or ".", exist_ok=True)
        formats.write_index(cache, ix)
        np.save(cache + "_queries.npy", q)
        np.save(cache + "_gt_ids.npy", gi)
        np.save(cache + "_gt_dists.npy", gd)
    return ix, q, gi, gd


def sweep(ix, q, gi, gd, mode, Ls, k, runs, log):
    rows = []
    Q = q.shape[0]
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=MODES[mode]) as e:
        e.load_index(ix)
        for L in Ls:
            e.set_searchparams(k, L)
            e.alloc(Q)
            times = []
            ids = None
            for r in range(runs + 1):                         # run 0: warm-up
                e.init(Q)
                t0 = time.perf_counter()
                ids, _ = e.query(q)
                dt = time.perf_counter() - t0
                if r:
                    times.append(dt)
            st = e.query_counters(Q)                          # iterations, candidates, dist_evals, fetched
            e.free()
            rec = O.recall(gi, gd, ids, k)
            row = {"mode": mode, "L": L, "recall": round(rec, 3), "qps_best": round(Q / min(times)), "qps_median": round(Q / float(np.median(times))),
                   "ms_best": round(1e3 * min(times), 3), "iterations": round(float(st[:, 0].mean()), 2), "evals": round(float(st[:, 2].mean()), 1),
                   "expanded": round(float(st[:, 1].mean()), 2)}
            log(json.dumps(row))
            rows.append(row)
        e.unload()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="sift1m", choices=sorted(WORKLOADS))
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--modes", default="pq,exact")
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=202)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0, help="recall (percent) the QPS comparison is taken at")
    ap.add_argument("--cache", default="", help="index prefix to write / reuse (formats.write_index + queries and ground truth as .npy)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    ix, q, gi, gd = workload(a.workload, a.queries, a.cache, log)
    out = {"workload": a.workload, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R), "Q": int(q.shape[0]),
           "k": k, "runs": a.runs, "rows": [], "at_target": {}}
    for mode in a.modes.split(","):
        rows = sweep(ix, q, gi, gd, mode, Ls, k, a.runs, log)
        out["rows"] += rows
        hit = [r for r in rows if r["recall"] >= a.target]
        out["at_target"][mode] = hit[0] if hit else None
        log(f"{mode}: smallest L with recall >= {a.target}: " + (f"L = {hit[0]['L']}, {hit[0]['qps_best']} queries/s" if hit else "none in the sweep"))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
