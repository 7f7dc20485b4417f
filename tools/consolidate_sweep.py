#!/usr/bin/env python3
"""What consolidation (Engine.consolidate) costs and what it does to recall and to the batch time, against the lazily masked graph
(Engine.set_excluded) of the SAME index in the SAME process.  Graph in HBM.

Workloads (tools/exact_sweep.py): structured synthetic 10^6-point indexes, SIFT1M-like (uint8, D = 128, m = 32) and DEEP-like (float, D = 96,
m = 74), R = 64.  Per workload and deletion rate (per cent of the ids, drawn at random with exclude_sweep's fixed seed) two engines hold the index:
MASKED keeps the set, CONSOLIDATED folds it into the graph at --alpha.

  cost     Engine.consolidate on a freshly loaded engine, --runs times: the whole call and its three parts (bang_get_consolidate_times: scan + list,
           the gather / sort / prune chunks, clear + seed list; host wall time around work that ends in a stream synchronise), rows rewritten, nodes
           removed, candidates dropped by the cut at 512.
  recall   10-recall@10 against brute force OVER THE LIVE POINTS (exclude_sweep.live_truth) over --Ls, masked against consolidated, on the
           self-paced PQ walk and on the exact walk (distance = 1).
  batch    ms per --batch queries (best and median of --runs bang_query calls after a warm-up; bang_init outside the timed region), masked
           (re-rank un-fused, bang_k_cand_live / bang_k_worklist_pick behind the walk) against consolidated (set empty, re-rank fused); the two
           engines alternate per L and run, so both see the same clocks.

There is no threshold: the numbers are a record.

  python tools/consolidate_sweep.py --workloads sift1m,deep1m --out profiles/consolidate.json --md profiles/consolidate_tables.md

Not part of bench.py: the measurement behind profiles/consolidate.md.
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
import exclude_sweep  # noqa: E402

WALKS = (("pq", 0), ("exact", 1))


def engine(ix):
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, capacity=int(ix.N))
    e.load_index(ix)
    return e


def cost(ix, ids, alpha, runs, log, workload, rate):
    """Engine.consolidate on a fresh load, `runs` times -> (rows of the cost table, the last engine: consolidated)"""
    rows, e = [], None
    for r in range(runs):
        if e is not None:
            e.close()
        e = engine(ix)
        e.set_excluded(ids)
        t0 = time.perf_counter()
        st = e.consolidate(alpha)
        wall = 1e3 * (time.perf_counter() - t0)
        row = dict(workload=workload, rate=rate, run=r, wall_ms=round(wall, 2), **{k + "_ms": round(v, 2) for k, v in e.consolidate_times().items()}, **st)
        log(json.dumps(row))
        rows.append(row)
    return rows, e


def batch(e, q, k, L, distance):
    e.set_option("distance", distance)
    e.set_option("search", 1)
    e.set_searchparams(k, L)
    e.alloc(q.shape[0])


def compare(masked, cons, q, truth, Ls, k, runs, log, workload, rate):
    rows = []
    gone = truth["gone"]
    for walk, distance in WALKS:
        for L in Ls:
            times = {"masked": [], "consolidated": []}
            ids = {}
            for name, e in (("masked", masked), ("consolidated", cons)):
                batch(e, q, k, L, distance)
            for r in range(runs + 1):                         # run 0: warm-up; the engines alternate
                for name, e in (("masked", masked), ("consolidated", cons)):
                    e.init(q.shape[0])
                    t0 = time.perf_counter()
                    ids[name], _ = e.query(q)
                    dt = time.perf_counter() - t0
                    if r:
                        times[name].append(dt)
            row = dict(workload=workload, rate=rate, walk=walk, L=L, Q=int(q.shape[0]))
            for name, e in (("masked", masked), ("consolidated", cons)):
                s = e.stats()
                e.free()
                assert not np.isin(ids[name], gone).any(), (name, "a deleted id was returned")
                row[name] = dict(recall=round(O.recall(truth["ids"], truth["dists"], ids[name], k), 3), ms_best=round(1e3 * min(times[name]), 3),
                                 ms_median=round(1e3 * float(np.median(times[name])), 3), rerank_fused=int(s["rerank_fused"]),
                                 exclude_launches=int(s["exclude_launches"]), excluded=int(s["excluded"]),
                                 padded=int((ids[name] == np.iinfo(np.uint64).max).sum()))
            log(json.dumps(row))
            rows.append(row)
    return rows


def markdown(out):
    s = []
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']}, D = {w['D']}, {w['dtype']}, m = {w['m']}, R = {w['R']}; alpha = {out['alpha']}, k = {out['k']}, "
              f"{out['runs']} runs per point", "",
              "| deleted % | run | call ms | scan + list | gather / sort / prune | clear + seed | rows rewritten | removed | dropped by the cut | still excluded |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        for r in (r for r in out["cost"] if r["workload"] == w["name"]):
            s.append(f"| {r['rate']:g} | {r['run']} | {r['total_ms']:.1f} | {r['scan_ms']:.1f} | {r['rows_ms']:.1f} | {r['clear_ms']:.1f} | {r['rows']} | "
                     f"{r['removed']} | {r['dropped']} | {r['still_excluded']} |")
        s += ["", f"{out['Q']} queries per batch; recall is 10-recall@10 against brute force over the live points", "",
              "| deleted % | walk | L | recall masked | recall consolidated | ms masked (best / median) | ms consolidated (best / median) | consolidated / masked | "
              "re-rank fused (masked / consolidated) |", "|---|---|---|---|---|---|---|---|---|"]
        for r in (r for r in out["rows"] if r["workload"] == w["name"]):
            a, b = r["masked"], r["consolidated"]
            s.append(f"| {r['rate']:g} | {r['walk']} | {r['L']} | {a['recall']:.2f} | {b['recall']:.2f} | {a['ms_best']:.3f} / {a['ms_median']:.3f} | "
                     f"{b['ms_best']:.3f} / {b['ms_median']:.3f} | {b['ms_best'] / a['ms_best']:.3f} | {a['rerank_fused']} / {b['rerank_fused']} |")
        s.append("")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--rates", default="1,10,30", help="deletion rates in per cent")
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cache", default="", help="directory of index prefixes to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("consolidate_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")]
    rates = [float(x) for x in a.rates.split(",") if x]
    out = {"k": k, "runs": a.runs, "alpha": a.alpha, "Q": a.batch, "rates": rates, "workloads": [], "cost": [], "rows": []}

    def flush():
        for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)

    for name in a.workloads.split(","):
        ix, q, _, _ = exact_sweep.workload(name, a.batch, os.path.join(a.cache, name) if a.cache else "", log)
        q = np.ascontiguousarray(q[:a.batch])
        out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R)})
        dev = torch.device("cuda", 0)
        for rate in rates:
            ids = exclude_sweep.random_ids(int(ix.N), rate)
            t0 = time.time()
            x = torch.from_numpy(ix.vectors().astype(np.float32)).to(dev)
            qq = torch.from_numpy(q.astype(np.float32)).to(dev)
            gi, gd = exclude_sweep.live_truth(x, qq, ids, k)
            del x, qq
            torch.cuda.empty_cache()
            log(f"{name}, {rate:g} % deleted: ground truth over the live points in {time.time() - t0:.1f} s")
            gone = ids[ids != ix.medoid]
            rows, cons = cost(ix, ids, a.alpha, a.runs, log, name, rate)
            out["cost"] += rows
            masked = engine(ix)
            masked.set_excluded(ids)
            out["rows"] += compare(masked, cons, q, dict(ids=gi, dists=gd, gone=gone), Ls, k, a.runs, log, name, rate)
            masked.close()
            cons.close()
            flush()                                           # (what is measured so far survives a time limit)
        del ix
    flush()


if __name__ == "__main__":
    main()
