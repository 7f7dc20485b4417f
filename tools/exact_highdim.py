#!/usr/bin/env python3
"""Exact distances in the walk (distance = 1) on the high-dimensional layouts -- GIST-like (float, D = 960, m = 120) and MNIST-like (uint8,
D = 784, m = 98) -- against the only other route for such indexes, the PQ walk through the LUT path (distance = 0), graph in HBM.

Structured synthetic indexes (bang_amd.synth), one query batch.  Per index: both modes over the L grid (tools/exact_sweep.py's sweep: recall,
queries/s, evaluations); then, at each mode's smallest L with 10-recall@10 >= --target, the two modes ALTERNATING, --runs launches each, and
the exact mode's vector bytes per second = evaluations x D x sizeof(T) / launch time.

Throughput bar (--bar): the wide float instance on the GIST-like index against the narrow float instance (the widest layout it runs, D = 256)
on a D = 256 float index of the same N, L and Q, alternating, --runs launches each; the spread of the narrow instance's launches is reported.

  python tools/exact_highdim.py --n 100000 --out profiles/exact_distance_highdim.json

Not part of bench.py: the measurement behind profiles/exact_distance_highdim.md.
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
from oracle import oracle as O  # noqa: E402
from tools import exact_sweep  # noqa: E402

# name: (D, dtype, m)
LAYOUTS = {"gist_like": (960, "float", 120), "mnist_like": (784, "uint8", 98), "f32_256": (256, "float", 64)}
TSIZE = {"float": 4, "uint8": 1, "int8": 1}


def build(name, N, R, Q, log):
    D, dtype, m = LAYOUTS[name]
    t0 = time.time()
    dev = "cuda" if bang_amd.device_count() > 0 else "cpu"
    ix, q, gi, gd = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=64, device=dev, pq_iters=4)
    log(f"built {name}: N={N} D={D} {dtype} R={R} m={m} Q={Q} in {time.time() - t0:.1f} s")
    return ix, q, gi, gd


class Runner:
    """One engine, one allocation; launch() times one bang_query (bang_init outside the timed region)."""
    def __init__(self, ix, q, mode, k, L):
        self.q, self.Q, self.D, self.ts = q, q.shape[0], int(ix.D), TSIZE[ix.dtype]
        self.e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=exact_sweep.MODES[mode])
        self.e.load_index(ix)
        self.e.set_searchparams(k, L)
        self.e.alloc(self.Q)
        self.launch()                                         # warm-up

    def launch(self):
        self.e.init(self.Q)
        t0 = time.perf_counter()
        self.ids, _ = self.e.query(self.q)
        return time.perf_counter() - t0

    def evals(self):
        return int(self.e.query_counters(self.Q)[:, 2].sum())

    def close(self):
        self.e.free()
        self.e.unload()
        self.e.close()


def alternate(a, b, runs):
    ta, tb = [], []
    for _ in range(runs):
        ta.append(a.launch())
        tb.append(b.launch())
    return ta, tb


def summary(times, r):
    ev = r.evals()
    gbs = [ev * r.D * r.ts / t / 1e9 for t in times]
    return {"ms": [round(1e3 * t, 3) for t in times], "qps_best": round(r.Q / min(times)), "qps_median": round(r.Q / float(np.median(times))),
            "evaluations": ev, "vector_GBps_best": round(max(gbs), 1), "vector_GBps_median": round(float(np.median(gbs)), 1),
            "vector_GBps_min": round(min(gbs), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--indexes", default="gist_like,mnist_like")
    ap.add_argument("--max-L", type=int, default=130)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0)
    ap.add_argument("--bar", type=int, default=1, help="1 = measure the throughput bar (wide float on D = 960 against narrow float on D = 256)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = list(range(k, a.max_L + 1, 12))
    out = {"N": a.n, "R": a.R, "Q": a.queries, "k": k, "runs": a.runs, "indexes": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    gist = None
    for name in [x for x in a.indexes.split(",") if x]:
        ix, q, gi, gd = build(name, a.n, a.R, a.queries, log)
        if name == "gist_like":
            gist = (ix, q)
        rec = {"D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "rows": [], "at_target": {}}
        for mode in ("exact", "pq"):
            rows = exact_sweep.sweep(ix, q, gi, gd, mode, Ls, k, 2, log)
            rec["rows"] += rows
            hit = [r for r in rows if r["recall"] >= a.target]
            rec["at_target"][mode] = hit[0] if hit else None
        if rec["at_target"]["exact"] and rec["at_target"]["pq"]:
            ex = Runner(ix, q, "exact", k, rec["at_target"]["exact"]["L"])
            pq = Runner(ix, q, "pq", k, rec["at_target"]["pq"]["L"])
            te, tp = alternate(ex, pq, a.runs)
            rec["alternating"] = {"exact": dict(summary(te, ex), L=rec["at_target"]["exact"]["L"], recall=round(O.recall(gi, gd, ex.ids, k), 3)),
                                  "pq": {"L": rec["at_target"]["pq"]["L"], "ms": [round(1e3 * t, 3) for t in tp], "qps_best": round(a.queries / min(tp)),
                                         "qps_median": round(a.queries / float(np.median(tp))), "recall": round(O.recall(gi, gd, pq.ids, k), 3)}}
            log(json.dumps({name: rec["alternating"]}))
            ex.close()
            pq.close()
        out["indexes"][name] = rec
        dump()
    if a.bar:
        if gist is None:
            gist = build("gist_like", a.n, a.R, a.queries, log)[:2]
        L = (out["indexes"].get("gist_like", {}).get("at_target", {}).get("exact") or {"L": 34})["L"]
        ix256, q256, _, _ = build("f32_256", a.n, a.R, a.queries, log)
        wide = Runner(gist[0], gist[1], "exact", k, L)
        narrow = Runner(ix256, q256, "exact", k, L)
        tw, tn = alternate(wide, narrow, max(a.runs, 5))
        sw, sn = summary(tw, wide), summary(tn, narrow)
        out["bar"] = {"L": L, "wide_d960": sw, "narrow_d256": sn,
                      "narrow_spread_GBps": round(sn["vector_GBps_best"] - sn["vector_GBps_min"], 1),
                      "met": bool(sw["vector_GBps_median"] >= sn["vector_GBps_median"] - (sn["vector_GBps_best"] - sn["vector_GBps_min"]))}
        log(json.dumps({"bar": out["bar"]}))
        wide.close()
        narrow.close()
    dump()


if __name__ == "__main__":
    main()
