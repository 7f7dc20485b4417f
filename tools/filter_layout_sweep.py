#!/usr/bin/env python3
"""The two visited-filter layouts (option filter_layout: 0 = split, 1 = word) on the SAME load of the SAME index in the SAME process: what
putting both bits of an id into one filter word does to launch time, recall and the number of distance evaluations (the false drops).

The option is read at bang_alloc, so one load serves both layouts; filter_layout = 0 is the parent's kernel, byte for byte, and every ratio
below is taken against it.  Workloads:

  sift1m     structured synthetic index (bang_amd.synth), uint8, D = 128, m = 32 -- graph in HBM
  sift70     the same vectors' layout with the 70-chunk PQ of the SIFT1B configuration, N = 1e6 -- graph in HBM
  shape      the shape-only 70-chunk index of tools/shape_workload.py (sift1b_shape: random graph, recall not meaningful), streamed, adjacency
             rows PULLED from host memory; --shape-n sets N (0 = the largest the machine holds)

Per workload, batch size (10 000 queries and a 1 250-query shard by default), L of the harness grid and layout: one warm-up bang_query and
--runs timed ones (bang_init outside the timed region, as the harness does); ms per batch (best and median of the timed runs), 10-recall@10,
dist_evals and fetched ids per query, filter_loads_skipped per query.  Then per workload and batch the smallest L with recall >= --target for
each layout and the time ratio there ("at equal recall").  The layouts alternate per L, so both see the same clocks and the same neighbours.
There is no threshold: the numbers are a record.

  python tools/filter_layout_sweep.py --workloads sift1m,sift70 --out profiles/filter_layout_sweep.json --md profiles/filter_layout_sweep.md
  python tools/filter_layout_sweep.py --workloads shape --shape-n 100000000 --shape-Ls 152 --runs 5

Not part of bench.py: the measurement behind profiles/filter_layout.md.
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
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402

exact_sweep.WORKLOADS.update({
    "sift70": (1_000_000, 128, "uint8", 64, 70, 256),        # the 70-chunk layout of the SIFT1B configuration at 1e6 points
})
LAYOUTS = (("split", bang_amd.FILTER_SPLIT), ("word", bang_amd.FILTER_WORD))


def measure(e, workload, q, gi, gd, batches, Ls, k, runs, log):
    rows = []
    for Q in batches:
        qb = np.ascontiguousarray(q[:Q])
        for L in Ls:
            for name, code in LAYOUTS:
                e.set_option("filter_layout", code)
                e.set_searchparams(k, L)
                e.alloc(Q)
                times, ids = [], None
                for r in range(runs + 1):                     # run 0: warm-up
                    e.init(Q)
                    t0 = time.perf_counter()
                    ids, _ = e.query(qb)
                    dt = time.perf_counter() - t0
                    if r:
                        times.append(dt)
                st = e.query_counters(Q)                      # iterations, candidates, dist_evals, fetched
                s = e.stats()
                e.free()
                assert int(s["filter_layout"]) == code and int(s["search_kernel"]) == 1, s
                row = {"workload": workload, "layout": name, "Q": Q, "L": L,
                       "recall": round(O.recall(gi[:Q], gd[:Q], ids, k), 3) if gi is not None else None,
                       "ms_best": round(1e3 * min(times), 4), "ms_median": round(1e3 * float(np.median(times)), 4),
                       "iterations": round(float(st[:, 0].mean()), 2), "expanded": round(float(st[:, 1].mean()), 2),
                       "evals": round(float(st[:, 2].mean()), 2), "fetched": round(float(st[:, 3].mean()), 2),
                       "filter_loads_skipped": round(int(s["filter_loads_skipped"]) / Q, 1), "graph_pull": int(s["graph_pull"]),
                       "rows_in_hbm": int(s["rows_in_hbm"]), "rerank_fused": int(s["rerank_fused"])}
                log(json.dumps(row))
                rows.append(row)
    return rows


def compare(rows, target):
    """Per (workload, Q): word against split at equal L, and at equal recall (each layout at its smallest L reaching the target)."""
    out = []
    for wq in sorted({(r["workload"], r["Q"]) for r in rows}):
        sel = [r for r in rows if (r["workload"], r["Q"]) == wq]
        by = {n: {r["L"]: r for r in sel if r["layout"] == n} for n, _ in LAYOUTS}
        at_L = {str(L): round(by["word"][L]["ms_best"] / by["split"][L]["ms_best"], 3) for L in sorted(by["word"]) if L in by["split"]}
        evals = {str(L): round(by["word"][L]["evals"] / by["split"][L]["evals"], 4) for L in sorted(by["word"]) if L in by["split"]}
        hit = {n: next((by[n][L] for L in sorted(by[n]) if by[n][L]["recall"] is not None and by[n][L]["recall"] >= target), None) for n, _ in LAYOUTS}
        out.append({"workload": wq[0], "Q": wq[1], "time_word_over_split_at_equal_L": at_L, "evals_word_over_split": evals,
                    "at_target": {n: h and {x: h[x] for x in ("L", "recall", "ms_best", "evals")} for n, h in hit.items()},
                    "time_word_over_split_at_equal_recall": round(hit["word"]["ms_best"] / hit["split"]["ms_best"], 3) if hit["word"] and hit["split"] else None})
    return out


def markdown(out):
    s = []
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']}, D = {w['D']}, {w['dtype']}, m = {w['m']}, R = {w['R']}; k = {out['k']}, {out['runs']} timed runs per point; {w['note']}", ""]
        for Q in sorted({r["Q"] for r in out["rows"] if r["workload"] == w["name"]}):
            sel = [r for r in out["rows"] if r["workload"] == w["name"] and r["Q"] == Q]
            s += [f"{Q} queries", "", "| L | layout | ms (best) | ms (median) | 10-recall@10 | dist_evals / query | fetched / query | filter loads skipped / query | time / split |",
                  "|---|---|---|---|---|---|---|---|---|"]
            base = {r["L"]: r["ms_best"] for r in sel if r["layout"] == "split"}
            for r in sorted(sel, key=lambda r: (r["L"], r["layout"])):
                rec = f"{r['recall']:.2f}" if r["recall"] is not None else "not meaningful"
                s.append(f"| {r['L']} | {r['layout']} | {r['ms_best']:.3f} | {r['ms_median']:.3f} | {rec} | {r['evals']} | {r['fetched']} | {r['filter_loads_skipped']} | "
                         f"{r['ms_best'] / base[r['L']]:.3f} |")
            s.append("")
    s += [f"At equal recall (smallest L with 10-recall@10 >= {out['target']} % per layout):", "",
          "| workload | queries | split: L | split: ms | word: L | word: ms | time word / split |", "|---|---|---|---|---|---|---|"]
    for c in out["compare"]:
        a, b = c["at_target"]["split"], c["at_target"]["word"]
        ratio = c["time_word_over_split_at_equal_recall"]
        s.append(f"| {c['workload']} | {c['Q']} | {a['L'] if a else 'not reached'} | {a['ms_best'] if a else '-'} | {b['L'] if b else 'not reached'} | "
                 f"{b['ms_best'] if b else '-'} | {ratio if ratio is not None else 'not measured'} |")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,sift70,shape")
    ap.add_argument("--batches", default="10000,1250")
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=154)
    ap.add_argument("--shape-Ls", default="152", help="worklist lengths of the shape-only workload (its recall is not meaningful)")
    ap.add_argument("--shape-n", type=int, default=0, help="points of the shape-only workload (0 = what the machine holds)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0, help="recall (percent) the equal-recall comparison is taken at")
    ap.add_argument("--cache", default="", help="directory of index prefixes to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    batches = [int(x) for x in a.batches.split(",")]
    out = {"k": k, "runs": a.runs, "target": a.target, "workloads": [], "rows": [], "compare": []}
    for name in a.workloads.split(","):
        if name == "shape":
            import torch
            from tools import shape_workload
            ix, q, _, _, d_codes, wl_name, _ = shape_workload.make("sift1b_shape", torch.device("cuda", 0), n_override=a.shape_n, Q=max(batches), log=log,
                                                                   stream=True)
            src = ix.entry_source
            with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1) as e:
                e.load_stream(ix, src[0], C.byref(src[1]), d_codes=d_codes, code_stride=getattr(ix, "code_stride", 0))
                out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R),
                                         "note": "shape-only (random graph and codes), streamed load, rows pulled by the kernel: " + wl_name})
                out["rows"] += measure(e, name, q, None, None, batches, [int(x) for x in a.shape_Ls.split(",")], k, a.runs, log)
                e.unload()
            shape_workload.release(ix)
            continue
        ix, q, gi, gd = exact_sweep.workload(name, max(batches), os.path.join(a.cache, name) if a.cache else "", log)
        with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
            e.load_index(ix)
            out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R),
                                     "note": "structured synthetic index, graph in HBM"})
            out["rows"] += measure(e, name, q, gi, gd, [b for b in batches if b <= q.shape[0]], Ls, k, a.runs, log)
            e.unload()
        del ix
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
