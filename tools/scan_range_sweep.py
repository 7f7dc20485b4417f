#!/usr/bin/env python3
"""What the exact range scan (Engine.scan_range) costs and what the walk's range search finds of its answer, on ONE load of ONE
index in ONE process.  Workloads (tools/exact_sweep.py): structured synthetic 10^6-point indexes, uint8 D = 128 (m = 32) and float D = 96 (m = 74).
Radii: every query's brute-force distance of rank 10 / 100 / 1000 (float vectors: times 1 + 1e-5).

  contenders      scan_range at each radius, Engine.scan at k = 100, the torch brute force (synth.knn to rank 1000: what tools/range_sweep.py
                  uses for its truth); they alternate, one warm-up and --runs timed calls each, medians; host wall time of the call
  pass split      count (+ prefix) / emit / sort of scan_range from the engine's event stamps, medians over the same calls
  range recall    the walk (distance = 1, option range_hits) at each L against scan_range's answer: the share of the true hits it returns

  python tools/scan_range_sweep.py --workloads sift1m,deep1m --md profiles/scan_range_sweep.md

Not part of bench.py: the measurement behind profiles/scan_range.md.  There is no threshold: the numbers are a record.
"""
import argparse
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
import exact_sweep  # noqa: E402

RANKS = (10, 100, 1000)


def timed(fn, runs):
    """median host milliseconds of runs calls behind one warm-up, and the last result"""
    out, t = None, []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        out = fn()
        if i:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--max-hits", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if bang_amd.device_count() < 1:
        raise SystemExit("scan_range_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    md = []
    log = lambda s: (print(s, flush=True), md.append(s))      # noqa: E731
    for name in a.workloads.split(","):
        ix, q, _, _ = exact_sweep.workload(name, a.batch, "", print)
        q = np.ascontiguousarray(q[:a.batch])
        Q = q.shape[0]
        dev = torch.device("cuda", 0)
        x, qq = torch.from_numpy(ix.vectors().astype(np.float32)).to(dev), torch.from_numpy(q.astype(np.float32)).to(dev)

        def brute():
            r = synth.knn(x, qq, max(RANKS))
            torch.cuda.synchronize()
            return r
        slack = np.float32(1.0 + 1e-5) if ix.dtype == "float" else np.float32(1.0)
        log(f"### {name}: N = {ix.N}, D = {ix.D}, {ix.dtype}; {Q} queries, max_hits = {a.max_hits}, medians of {a.runs}\n")
        log("| call | ms (host) | count + prefix ms | emit ms | sort ms | hits per query | truncated queries |\n|---|---|---|---|---|---|---|")
        truth = {}
        with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE) as e:
            e.load_index(ix)
            ms_b, (_, td) = timed(brute, a.runs)
            td = td.cpu().numpy().astype(np.float32)
            radii = {n: np.ascontiguousarray(td[:, n - 1] * slack, np.float32) for n in RANKS}
            ms_s, _ = timed(lambda: e.scan(q, 100), a.runs)
            for n in RANKS:                                       # (the contenders alternate: every call sees the same clocks)
                split = []

                def ranged():
                    r = e.scan_range(q, radii[n], a.max_hits)
                    split.append((e.scan_range_times()["count"], e.scan_range_times()["emit"], e.scan_times()["merge"]))
                    return r
                ms, truth[n] = timed(ranged, a.runs)
                c, em, so = np.median(np.array(split[1:]), axis=0)
                cnt = np.diff(truth[n][0].astype(np.int64))
                log(f"| scan_range, rank {n} | {ms:.2f} | {c:.2f} | {em:.2f} | {so:.2f} | {cnt.mean():.1f} | {int((truth[n][3] > a.max_hits).sum())} |")
                timed(brute, 1), timed(lambda: e.scan(q, 100), 1)
            log(f"| scan, k = 100 | {ms_s:.2f} | - | - | - | - | - |\n| torch brute force to rank 1000 | {ms_b:.2f} | - | - | - | - | - |\n")
            e.unload()
        del x, qq
        torch.cuda.empty_cache()
        log("| L | " + " | ".join(f"range recall %, rank {n}" for n in RANKS) + " |\n|---|" + "---|" * len(RANKS))
        with bang_amd.Engine(ix.dtype, distance=1, graph=bang_amd.GRAPH_DEVICE, range_hits=a.max_hits) as e:
            e.load_index(ix)
            for L in (int(v) for v in a.Ls.split(",")):
                cells = []
                for n in RANKS:
                    e.set_searchparams(10, L)
                    e.alloc(Q)
                    e.set_radii(radii[n])
                    e.init(Q)
                    e.query(q)
                    lims, ids, _ = e.range_results(Q)
                    e.free()
                    tl, ti = truth[n][0], truth[n][1]
                    found = sum(np.intersect1d(ids[int(lims[i]):int(lims[i + 1])], ti[int(tl[i]):int(tl[i + 1])], assume_unique=True).size for i in range(Q))
                    cells.append(f"{100.0 * found / max(int(tl[-1]), 1):.2f}")
                log(f"| {L} | " + " | ".join(cells) + " |")
            e.unload()
        log("")
        if a.md:
            with open(a.md, "w") as f:
                f.write("\n".join(md) + "\n")
        del ix


if __name__ == "__main__":
    main()
