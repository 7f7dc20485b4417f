#!/usr/bin/env python3
"""What excluded ids (lazy deletes: Engine.set_excluded) cost and what they do to recall, on the SAME load of the SAME index in the
SAME process.  The set is consumed at bang_alloc and the walk never reads it, so one load serves every column:

  default      the parent's run: X empty, the re-rank fused into the search launch where it can be
  unfused      X empty, fuse_rerank = 0: the re-rank a launch of its own -- the cost of un-fusing alone
  X = r %      r per cent of the ids, drawn at random with a fixed seed: bang_k_cand_live + the re-rank launch on the live list
  exact        distance = 1, X empty (--exact): the exact-distance kernel writes its k results itself
  exact X = r  distance = 1: the kernel hands over its whole worklist (rr_k = L), bang_k_worklist_pick takes the first k live entries

Workloads (tools/exact_sweep.py): structured synthetic indexes, SIFT1M-like (uint8, D = 128) and DEEP-like (float, D = 96); graph in HBM, and graph
in host RAM with the rows pulled by the kernel (pull = 1, no HBM row copy).  Per workload, placement, batch size, L of the harness grid and
column: one warm-up bang_query and --runs timed ones (bang_init outside the timed region); ms per batch (best and median: host wall time of
bang_query), launches, and 10-recall@10 against ground truth RECOMPUTED OVER THE LIVE POINTS ONLY (synth.knn on the points not in X).  The
columns alternate per L, so all see the same clocks.  Then per deletion rate the smallest L reaching --target, and the margin of each masked
column over `unfused` at equal L.  There is no threshold: the numbers are a record.

  python tools/exclude_sweep.py --workloads sift1m,deep1m --out profiles/exclude_sweep.json --md profiles/exclude_sweep.md

Kernel times of bang_k_cand_live / bang_k_worklist_pick beside the re-rank and search launches come from a profiler run of their own over one
point (the tool is the profiled program), e.g.

  rocprofv3 --kernel-trace --stats -d out -- python tools/exclude_sweep.py --workloads sift1m --batches 10000 --Ls 58 --rates 10 --exact --no-recall

Not part of bench.py: the measurement behind profiles/exclude.md.
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
from bang_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402

SEED = 20240


def random_ids(N, rate):
    """rate per cent of the ids 0 .. N - 1, sorted; the same ids for the same (N, rate)."""
    return np.sort(np.random.default_rng(SEED + int(rate * 100)).choice(N, size=int(N * rate / 100.0), replace=False)).astype(np.uint32)


def live_truth(vectors, queries, excluded, k):
    """Ground truth over the points NOT in `excluded` (torch tensors on any device): -> (ids u32 [Q][k] in the index's numbering, dists f32)"""
    import torch
    keep = torch.ones(vectors.shape[0], dtype=torch.bool, device=vectors.device)
    if len(excluded):
        keep[torch.from_numpy(excluded.astype(np.int64)).to(vectors.device)] = False
    live = keep.nonzero().squeeze(1)
    ids, d = synth.knn(vectors[live], queries, k)
    return live[ids].cpu().numpy().astype(np.uint32), d.cpu().numpy().astype(np.float32)


def columns(rates, exact):
    cols = [("default", dict(), None), ("unfused", dict(fuse_rerank=0), None)]
    cols += [(f"X = {r:g} %", dict(), r) for r in rates]
    if exact:
        cols += [("exact", dict(distance=1), None)] + [(f"exact X = {r:g} %", dict(distance=1), r) for r in rates]
    return cols


def measure(e, workload, placement, N, q, truth, batches, Ls, k, runs, cols, log):
    rows = []
    for Q in batches:
        qb = np.ascontiguousarray(q[:Q])
        for L in Ls:
            for name, opts, rate in cols:
                for key in ("fuse_rerank", "distance"):
                    e.set_option(key, opts.get(key, -1 if key == "fuse_rerank" else 0))
                if rate is None:
                    e.clear_excluded()
                else:
                    e.set_excluded(random_ids(N, rate))
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
                assert int(s["exclude_launches"]) == (0 if rate is None else 1) and int(s["search_kernel"]) == 1, s
                gt = truth.get(rate or 0)
                row = {"workload": workload, "placement": placement, "column": name, "rate": rate or 0, "exact": int("distance" in opts), "Q": Q, "L": L,
                       "recall": round(O.recall(gt[0][:Q], gt[1][:Q], ids, k), 3) if gt is not None else None,
                       "ms_best": round(1e3 * min(times), 4), "ms_median": round(1e3 * float(np.median(times)), 4),
                       "expanded": round(float(st[:, 1].mean()), 2), "evals": round(float(st[:, 2].mean()), 2),
                       "rerank_fused": int(s["rerank_fused"]), "exclude_launches": int(s["exclude_launches"]), "excluded": int(s["excluded"]),
                       "padded": int((ids == np.iinfo(np.uint64).max).sum())}
                log(json.dumps(row))
                rows.append(row)
    e.clear_excluded()
    for key, v in (("fuse_rerank", -1), ("distance", 0)):
        e.set_option(key, v)
    return rows


def compare(rows, target):
    """Per (workload, placement, Q): each masked column over `unfused` (PQ) / `exact` (distance = 1) at equal L, and the smallest L reaching the target."""
    out = []
    for key in sorted({(r["workload"], r["placement"], r["Q"]) for r in rows}):
        sel = [r for r in rows if (r["workload"], r["placement"], r["Q"]) == key]
        by = {}
        for r in sel:
            by.setdefault(r["column"], {})[r["L"]] = r
        c = {"workload": key[0], "placement": key[1], "Q": key[2], "over_base_at_equal_L": {}, "smallest_L_at_target": {}}
        for col, at in by.items():
            base = by.get("exact" if col.startswith("exact") else "unfused", {})
            if col not in ("default", "exact"):
                c["over_base_at_equal_L"][col] = {str(L): round(at[L]["ms_best"] / base[L]["ms_best"], 3) for L in sorted(at) if L in base}
            hit = next((at[L] for L in sorted(at) if at[L]["recall"] is not None and at[L]["recall"] >= target), None)
            c["smallest_L_at_target"][col] = hit and {x: hit[x] for x in ("L", "recall", "ms_best")}
        if "default" in by and "unfused" in by:
            c["unfused_over_default"] = {str(L): round(by["unfused"][L]["ms_best"] / by["default"][L]["ms_best"], 3) for L in sorted(by["unfused"]) if L in by["default"]}
        out.append(c)
    return out


def markdown(out):
    s = []
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']}, D = {w['D']}, {w['dtype']}, m = {w['m']}, R = {w['R']}; k = {out['k']}, {out['runs']} timed runs per point", ""]
        for placement in ("device", "host"):
            for Q in sorted({r["Q"] for r in out["rows"] if r["workload"] == w["name"] and r["placement"] == placement}):
                sel = [r for r in out["rows"] if r["workload"] == w["name"] and r["placement"] == placement and r["Q"] == Q]
                note = "graph = device" if placement == "device" else "graph = host (pull = 1, every row over PCIe)"
                s += [f"{note}, {Q} queries", "", "| L | column | ms (best) | ms (median) | 10-recall@10 (live points) | re-rank fused | exclude launches | time / base |",
                      "|---|---|---|---|---|---|---|---|"]
                base = {(r["L"], r["exact"]): r["ms_best"] for r in sel if r["column"] in ("unfused", "exact")}
                for r in sel:
                    rec = f"{r['recall']:.2f}" if r["recall"] is not None else "not measured"
                    b = base.get((r["L"], r["exact"]))
                    s.append(f"| {r['L']} | {r['column']} | {r['ms_best']:.3f} | {r['ms_median']:.3f} | {rec} | {r['rerank_fused']} | {r['exclude_launches']} | "
                             f"{r['ms_best'] / b:.3f} |" if b else f"| {r['L']} | {r['column']} | {r['ms_best']:.3f} | {r['ms_median']:.3f} | {rec} | - | - | - |")
                s.append("")
    s += [f"Smallest L of the grid with 10-recall@10 >= {out['target']} % (ground truth over the live points), per column:", "",
          "| workload | graph | queries | column | L | recall | ms |", "|---|---|---|---|---|---|---|"]
    for c in out["compare"]:
        for col, h in c["smallest_L_at_target"].items():
            s.append(f"| {c['workload']} | {c['placement']} | {c['Q']} | {col} | {h['L'] if h else 'not reached'} | {h['recall'] if h else '-'} | {h['ms_best'] if h else '-'} |")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--placements", default="device,host")
    ap.add_argument("--batches", default="1250,10000")
    ap.add_argument("--Ls", default="", help="comma-separated worklist lengths (default: the harness grid 10, 22, ... up to --max-L)")
    ap.add_argument("--max-L", type=int, default=106)
    ap.add_argument("--rates", default="1,10,30", help="deletion rates in per cent")
    ap.add_argument("--exact", action="store_true", help="add the distance = 1 columns (bang_k_worklist_pick)")
    ap.add_argument("--no-recall", action="store_true", help="skip the ground truth over the live points (a profiler run)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--target", type=float, default=90.0)
    ap.add_argument("--cache", default="", help="directory of index prefixes to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("exclude_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")] if a.Ls else list(range(k, a.max_L + 1, 12))
    batches = [int(x) for x in a.batches.split(",")]
    rates = [float(x) for x in a.rates.split(",") if x]
    cols = columns(rates, a.exact)
    out = {"k": k, "runs": a.runs, "target": a.target, "rates": rates, "workloads": [], "rows": [], "compare": []}
    for name in a.workloads.split(","):
        ix, q, gi, gd = exact_sweep.workload(name, max(batches), os.path.join(a.cache, name) if a.cache else "", log)
        truth = {}
        if not a.no_recall:
            t0 = time.time()
            dev = torch.device("cuda", 0)
            x = torch.from_numpy(ix.vectors().astype(np.float32)).to(dev)
            qq = torch.from_numpy(q.astype(np.float32)).to(dev)
            truth[0] = (np.ascontiguousarray(gi, dtype=np.uint32), np.ascontiguousarray(gd, dtype=np.float32))
            for r in rates:
                truth[r] = live_truth(x, qq, random_ids(ix.N, r), k)
            del x, qq
            torch.cuda.empty_cache()
            log(f"ground truth over the live points for {rates} % deleted: {time.time() - t0:.1f} s")
        out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R)})
        for placement in a.placements.split(","):
            opts = dict(graph=bang_amd.GRAPH_DEVICE) if placement == "device" else dict(graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0)
            with bang_amd.Engine(ix.dtype, **opts) as e:
                e.load_index(ix)
                out["rows"] += measure(e, name, placement, int(ix.N), q, truth, [b for b in batches if b <= q.shape[0]], Ls, k, a.runs, cols, log)
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
