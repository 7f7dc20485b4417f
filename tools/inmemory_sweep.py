#!/usr/bin/env python3
"""The BANG_Base walk (semantics = 0) against the BANG_Inmemory walk (semantics = 1) over an L sweep, graph in HBM.

Builds a structured synthetic index (bang_amd.synth: kNN + random-link graph, trained PQ, brute-force ground truth), then for each mode and
each L runs the engine on the whole query batch: one warm-up run and --runs timed bang_query calls (bang_init outside the timed region, as the
harness does).  Reports per mode and L: 10-recall@10, QPS (best and median of the timed runs), mean and p99 iterations per query, and the time
per iteration -- the best timed bang_query divided by the batch's total iterations (the modes' caps differ, L + 49 / L + 119, so QPS alone does
not compare the kernels).  Per L it also reports the share of queries whose result ids differ between the two modes.

  python tools/inmemory_sweep.py --workload sift --out inmemory_sift.json
  python tools/inmemory_sweep.py --workload deep --Ls 46 --runs 1

Not part of bench.py: the measurement behind profiles/inmemory_semantics.md.
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
    "sift": (200_000, 128, "uint8", 64, 32, 256),       # SIFT1M-like layout (uint8, D = 128, m = 32)
    "deep": (200_000, 96, "float", 64, 74, 256),        # DEEP-like layout (float, D = 96, m = 74)
    "small": (50_000, 128, "uint8", 64, 32, 64),
}
MODES = {"base": bang_amd.SEMANTICS_BASE, "inmemory": bang_amd.SEMANTICS_INMEMORY}


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
    rows, ids_by_L = [], {}
    Q = q.shape[0]
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, semantics=MODES[mode]) as e:
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
            its = st[:, 0].astype(np.float64)
            row = {"mode": mode, "L": L, "recall": round(rec, 3), "qps_best": round(Q / min(times)), "qps_median": round(Q / float(np.median(times))),
                   "ms_best": round(1e3 * min(times), 3), "iterations": round(float(its.mean()), 2), "iterations_p99": float(np.percentile(its, 99)),
                   "us_per_iteration": round(1e6 * min(times) / float(its.sum()), 5), "evals": round(float(st[:, 2].mean()), 1)}
            log(json.dumps(row))
            rows.append(row)
            ids_by_L[L] = ids
        e.unload()
    return rows, ids_by_L


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="sift", choices=sorted(WORKLOADS))
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--modes", default="base,inmemory")
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=154)
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
    ids = {}
    for mode in a.modes.split(","):
        rows, ids[mode] = sweep(ix, q, gi, gd, mode, Ls, k, a.runs, log)
        out["rows"] += rows
        hit = [r for r in rows if r["recall"] >= a.target]
        out["at_target"][mode] = hit[0] if hit else None
        log(f"{mode}: smallest L with recall >= {a.target}: " + (f"L = {hit[0]['L']}, {hit[0]['qps_best']} queries/s" if hit else "none in the sweep"))
    if len(ids) == 2:
        a_, b_ = list(ids.values())
        out["ids_differ"] = {L: round(float((a_[L] != b_[L]).any(axis=1).mean()), 4) for L in Ls}
        log("share of queries whose ids differ between the modes: " + json.dumps(out["ids_differ"]))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
