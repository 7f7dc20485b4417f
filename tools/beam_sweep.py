#!/usr/bin/env python3
"""Exact-distance search (distance = 1) at beam = 1, 2, 3 and 4 on the SAME index: what expanding up to four parents per iteration does to
recall, iterations and launch time.

Builds the structured synthetic index of tools/exact_sweep.py (bang_amd.synth), then for each placement -- graph = device, and graph = host
with pull = 1 (no HBM row copy: every row over PCIe) --, each beam, each batch size and each L of the harness grid runs the engine: one warm-up
run and --runs timed bang_query calls (bang_init outside the timed region, as the harness does).  beam = 1 runs the kernels of
bang_search_exact.hip, beam > 1 those of bang_search_beam.hip; everything else about the engine is the same.

Per point: 10-recall@10, queries/s and milliseconds (best and median of the timed runs), mean iterations, expansions and distance evaluations
per query.  Per placement, batch and beam > 1 the comparison against beam = 1 IN THE SAME RUN: the ratio of the best times at equal L, and at
equal recall -- each beam at its smallest L with recall >= --target.  There is no threshold: the numbers are a record.

  python tools/beam_sweep.py --workload sift1m --out profiles/exact_beam_sift1m.json --md profiles/exact_beam_sift1m.md
  python tools/beam_sweep.py --workload small --placements device --batches 64 --Ls 10,22,34 --runs 2          (a quick look)

Not part of bench.py: the measurement behind profiles/exact_beam.md.
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
from oracle import oracle as O  # noqa: E402
from tools.exact_sweep import WORKLOADS, workload  # noqa: E402

PLACEMENTS = {
    "device": dict(graph=bang_amd.GRAPH_DEVICE),
    "host": dict(graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0),
}


def sweep(ix, q, gi, gd, placement, beam, batches, Ls, k, runs, log):
    rows = []
    with bang_amd.Engine(ix.dtype, distance=bang_amd.DISTANCE_EXACT, beam=beam, **PLACEMENTS[placement]) as e:
        e.load_index(ix)
        for Q in batches:
            qb = np.ascontiguousarray(q[:Q])
            for L in Ls:
                e.set_searchparams(k, L)
                e.alloc(Q)
                times = []
                ids = None
                for r in range(runs + 1):                     # run 0: warm-up
                    e.init(Q)
                    t0 = time.perf_counter()
                    ids, _ = e.query(qb)
                    dt = time.perf_counter() - t0
                    if r:
                        times.append(dt)
                st = e.query_counters(Q)                      # iterations, candidates, dist_evals, fetched
                e.free()
                rec = O.recall(gi[:Q], gd[:Q], ids, k)
                row = {"placement": placement, "beam": beam, "Q": Q, "L": L, "recall": round(rec, 3), "qps_best": round(Q / min(times)),
                       "qps_median": round(Q / float(np.median(times))), "ms_best": round(1e3 * min(times), 4),
                       "ms_median": round(1e3 * float(np.median(times)), 4), "iterations": round(float(st[:, 0].mean()), 2),
                       "expanded": round(float(st[:, 1].mean()), 2), "evals": round(float(st[:, 2].mean()), 1)}
                log(json.dumps(row))
                rows.append(row)
        e.unload()
    return rows


def compare(rows, target):
    """Per (placement, Q, beam > 1): times against beam = 1 at equal L, and at equal recall (each at its smallest L reaching the target)."""
    out = []
    key = lambda r: (r["placement"], r["Q"])                 # noqa: E731
    for pq in sorted({key(r) for r in rows}):
        sel = [r for r in rows if key(r) == pq]
        base = {r["L"]: r for r in sel if r["beam"] == 1}
        if not base:
            continue
        hit1 = next((base[L] for L in sorted(base) if base[L]["recall"] >= target), None)
        for beam in sorted({r["beam"] for r in sel} - {1}):
            mine = {r["L"]: r for r in sel if r["beam"] == beam}
            at_L = {str(L): round(mine[L]["ms_best"] / base[L]["ms_best"], 3) for L in sorted(mine) if L in base}
            hit = next((mine[L] for L in sorted(mine) if mine[L]["recall"] >= target), None)
            out.append({"placement": pq[0], "Q": pq[1], "beam": beam, "time_ratio_at_equal_L": at_L,
                        "at_target_beam1": hit1 and {x: hit1[x] for x in ("L", "recall", "ms_best", "iterations")},
                        "at_target": hit and {x: hit[x] for x in ("L", "recall", "ms_best", "iterations")},
                        "time_ratio_at_equal_recall": round(hit["ms_best"] / hit1["ms_best"], 3) if hit and hit1 else None})
    return out


def markdown(out):
    s = [f"### {out['workload']}: N = {out['N']}, D = {out['D']}, {out['dtype']}, R = {out['R']}; k = {out['k']}, {out['runs']} timed runs per point", ""]
    for placement in sorted({r["placement"] for r in out["rows"]}):
        for Q in sorted({r["Q"] for r in out["rows"]}):
            sel = [r for r in out["rows"] if r["placement"] == placement and r["Q"] == Q]
            if not sel:
                continue
            s += [f"graph = {placement}{' (pull = 1, every row over PCIe)' if placement == 'host' else ''}, {Q} queries", "",
                  "| L | beam | 10-recall@10 | ms (best) | queries/s | iterations | expanded | evaluations | time / beam 1 |", "|---|---|---|---|---|---|---|---|---|"]
            base = {r["L"]: r["ms_best"] for r in sel if r["beam"] == 1}
            for r in sorted(sel, key=lambda r: (r["L"], r["beam"])):
                ratio = f"{r['ms_best'] / base[r['L']]:.2f}" if r["L"] in base else "not measured"
                s.append(f"| {r['L']} | {r['beam']} | {r['recall']:.2f} | {r['ms_best']:.3f} | {r['qps_best']} | {r['iterations']} | {r['expanded']} | {r['evals']} | {ratio} |")
            s.append("")
    s += [f"At equal recall (smallest L with 10-recall@10 >= {out['target']} % per beam):", "",
          "| graph | queries | beam | L | ms | beam 1: L | beam 1: ms | time / beam 1 |", "|---|---|---|---|---|---|---|---|"]
    for c in out["compare"]:
        a, b = c["at_target"], c["at_target_beam1"]
        s.append(f"| {c['placement']} | {c['Q']} | {c['beam']} | {a['L'] if a else 'not reached'} | {a['ms_best'] if a else '-'} | {b['L'] if b else 'not reached'} | "
                 f"{b['ms_best'] if b else '-'} | {c['time_ratio_at_equal_recall'] if c['time_ratio_at_equal_recall'] is not None else 'not measured'} |")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="sift1m", choices=sorted(WORKLOADS))
    ap.add_argument("--placements", default="device,host")
    ap.add_argument("--beams", default="1,2,3,4")
    ap.add_argument("--batches", default="64,1250,10000")
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=202)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0, help="recall (percent) the equal-recall comparison is taken at")
    ap.add_argument("--cache", default="", help="index prefix to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    batches = [int(x) for x in a.batches.split(",")]
    ix, q, gi, gd = workload(a.workload, max(batches), a.cache, log)
    out = {"workload": a.workload, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R), "k": k, "runs": a.runs,
           "target": a.target, "rows": [], "compare": []}
    for placement in a.placements.split(","):
        for beam in (int(x) for x in a.beams.split(",")):
            out["rows"] += sweep(ix, q, gi, gd, placement, beam, [b for b in batches if b <= q.shape[0]], Ls, k, a.runs, log)
    out["compare"] = compare(out["rows"], a.target)
    for c in out["compare"]:
        log(json.dumps(c))
    for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
