#!/usr/bin/env python3
"""Exact-distance search (distance = 1, graph in HBM) on the any-dimension layouts of option any_dim against their aligned neighbours.

Two groups of structured synthetic indexes (bang_amd.synth, --points each), all engines of a group alive in ONE process:

  int8    D = 100 (any_dim = 1: search_exact_anydim_kernel)   against   D = 96 and D = 128 (today's narrow instances)
  float   D = 201, MIPS parameters, queries of 200 floats (any_dim = 1)   against   D = 200, L2 (today's narrow instance)

For each L the engines of a group run the whole query batch in turn, alternating, --runs times (one warm-up round first; bang_init outside the
timed region); reported per layout: the median time, queries/s, mean iterations and distance evaluations per query, and the ratio of the median
to that of the any-dimension layout's neighbours.  The indexes differ (each layout has its own vectors and graph), so the evaluations per query
are printed beside the times.

  python tools/anydim_sweep.py --out anydim.json

Not part of bench.py: the measurement behind profiles/exact_anydim.md.  Not measured here: the pulled placement, the tile path (D > 256),
profiler kernel times.
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
from bang_amd import synth  # noqa: E402

# group -> [(label, D, dtype, any_dim, MIPS)]: the first entry is the any-dimension layout, the others its neighbours
GROUPS = {
    "int8": [("i8_100", 100, "int8", 1, False), ("i8_96", 96, "int8", 0, False), ("i8_128", 128, "int8", 0, False)],
    "float": [("f32_201_mips", 201, "float", 1, True), ("f32_200", 200, "float", 0, False)],
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--groups", default="int8,float")
    ap.add_argument("--Ls", default="22,46,94")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k, R = 10, 64
    Ls = [int(x) for x in a.Ls.split(",")]
    dev = "cuda" if bang_amd.device_count() > 0 else "cpu"
    out = {"N": a.points, "Q": a.queries, "k": k, "R": R, "runs": a.runs, "rows": []}
    for group in a.groups.split(","):
        engines = []
        for label, D, dtype, any_dim, mips in GROUPS[group]:
            t0 = time.time()
            ix, q, _, _ = synth.make_index(a.points, D, dtype, R, max(1, D // 4), a.queries, K=k, n_clusters=256, device=dev, pq_iters=1)
            log(f"built {label}: N={a.points} D={D} {dtype} R={R} in {time.time() - t0:.1f} s")
            e = bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT, any_dim=any_dim)
            e.load_index(ix)
            engines.append((label, e, np.ascontiguousarray(q[:, :D - 1] if mips else q), bang_amd.DIST_MIPS if mips else bang_amd.DIST_L2))
            del ix
        for L in Ls:
            times = {label: [] for label, _, _, _ in engines}
            for _, e, q, fn in engines:
                e.set_searchparams(k, L, fn)
                e.alloc(a.queries)
            for r in range(a.runs + 1):                       # round 0: warm-up
                for label, e, q, _ in engines:                # alternating: one batch per layout per round
                    e.init(a.queries)
                    t0 = time.perf_counter()
                    e.query(q)
                    if r:
                        times[label].append(time.perf_counter() - t0)
            med0 = float(np.median(times[engines[0][0]]))
            for label, e, q, _ in engines:
                st = e.query_counters(a.queries)              # iterations, candidates, dist_evals, fetched
                e.free()
                med = float(np.median(times[label]))
                row = {"group": group, "layout": label, "L": L, "ms_median": round(1e3 * med, 3), "qps_median": round(a.queries / med),
                       "iterations": round(float(st[:, 0].mean()), 2), "evals": round(float(st[:, 2].mean()), 1),
                       "anydim_over_this": round(med0 / med, 3)}
                log(json.dumps(row))
                out["rows"].append(row)
        for _, e, _, _ in engines:
            e.unload()
            e.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
