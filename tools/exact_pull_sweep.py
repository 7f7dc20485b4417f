#!/usr/bin/env python3
"""Exact distances in the walk against the PQ walk + re-rank when the adjacency rows are PULLED by the kernel (graph = host, pull = 1).

Builds a structured synthetic index (tools/exact_sweep.py's builder and cache), loads it ONCE in host placement and runs, on that load:

  pq-pull        distance = 0, every row over PCIe            exact-pull        distance = 1, every row over PCIe
  pq-rows-hbm    distance = 0, all rows in the HBM row copy   exact-rows-hbm    distance = 1, all rows in the HBM row copy

(the option `distance` is read at bang_alloc, so both modes share the load; bang_rows_slice_e(0, N) puts the rows into HBM between the two
halves), then loads it once more with graph = device for `exact-device` and `pq-device`.  Per configuration and L: one warm-up bang_query and
--runs timed ones on the whole batch (bang_init outside the timed region), 10-recall@10, mean iterations / evaluations per query and the
pulled bytes per query (bang_get_stats).  Then per configuration the smallest L with recall >= --target.

  python tools/exact_pull_sweep.py --workload sift200k --out exact_pull_sift200k.json

Not part of bench.py: the measurement behind profiles/exact_distance_pull.md.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bang_amd  # noqa: E402
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402

# the layouts of profiles/exact_distance.md at an N one sitting builds and sweeps
exact_sweep.WORKLOADS.update({
    "sift200k": (200_000, 128, "uint8", 64, 32, 128),
    "deep200k": (200_000, 96, "float", 64, 74, 128),
})
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
        st = e.query_counters(Q)                              # iterations, candidates, dist_evals, fetched
        s = e.stats()
        e.free()
        row = {"config": name, "mode": mode, "L": L, "recall": round(O.recall(gi, gd, ids, k), 3), "qps_best": round(Q / min(times)),
               "qps_median": round(Q / float(np.median(times))), "ms_best": round(1e3 * min(times), 3),
               "iterations": round(float(st[:, 0].mean()), 2), "evals": round(float(st[:, 2].mean()), 1),
               "expanded": round(float(st[:, 1].mean()), 2), "pulled_bytes_per_query": round(int(s["pulled_bytes"]) / Q, 1),
               "graph_pull": int(s["graph_pull"]), "rows_in_hbm": int(s["rows_in_hbm"]), "rerank_fused": int(s["rerank_fused"])}
        log(json.dumps(row))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="sift200k", choices=sorted(exact_sweep.WORKLOADS))
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=94)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0)
    ap.add_argument("--cache", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    ix, q, gi, gd = exact_sweep.workload(a.workload, a.queries, a.cache, log)
    out = {"workload": a.workload, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R), "Q": int(q.shape[0]),
           "k": k, "runs": a.runs, "rows": [], "at_target": {}}
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0) as e:     # ONE load: both modes, both row sources
        e.load_index(ix)
        for mode in ("pq", "exact"):
            out["rows"] += measure(e, f"{mode}-pull", mode, q, gi, gd, Ls, k, a.runs, log)
        e.rows_slice(0, ix.N)
        for mode in ("exact", "pq"):
            out["rows"] += measure(e, f"{mode}-rows-hbm", mode, q, gi, gd, Ls, k, a.runs, log)
        e.unload()
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
        e.load_index(ix)
        for mode in ("exact", "pq"):
            out["rows"] += measure(e, f"{mode}-device", mode, q, gi, gd, Ls, k, a.runs, log)
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
