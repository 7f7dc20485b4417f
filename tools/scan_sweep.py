"""The exact scan against what it replaces: python tools/scan_sweep.py [--workloads sift1m,deep1m] [--out profiles/scan.md]

One process, one GPU, the structured 10^6-point indexes of tools/exact_sweep.py (uint8 m = 32, float m = 74).  Per workload, the contenders run
alternately, one warm-up and five timed runs each, medians recorded:

  * Engine.scan for Q = 100 and 10 000 at k = 10 and 100, split into scan launches and merge (Engine.scan_times)
  * the same truth by bang_amd.synth.knn on the same GPU -- what the tools use today -- and how many of its ids differ from the scan's, tie-aware
    (an id of the scan's answer is missed when synth.knn neither lists it nor lists the scan's k-th distance in its place)
  * the exact-distance walk at the smallest L of the list that reaches 90 % 10-recall@10 against the scan
  * label shares 50 / 10 / 1 % (tools/labels_sweep.py's table): the scan's time beside the filtered walk's time and its recall against the scan
  * the 8-bit kernel's share of the i8 MFMA rate: 2 N Q D operations over the scan launches' time, against 2 x the dense BF16 rate of the chip
"""
import argparse
import datetime
import json
import os
import subprocess
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
import labels_sweep  # noqa: E402

RUNS = 5
I8_PEAK_OPS = 2 * 2.5e15            # i8 MFMA = 2 x the dense BF16 rate (MI355X: 2.5 PFLOP/s BF16)
SHARES = (50, 10, 1)
WALK_LS = (10, 14, 20, 28, 40, 56, 80, 112, 160)


def median_ms(fn, runs=RUNS):
    fn()                                                  # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def alternate_ms(fns, runs=RUNS):
    """the contenders in turn, run after run: one warm-up each, then the median of `runs` per contender"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(t)) for t in ts]


def missed(scan_ids, scan_d, knn_ids):
    """ids of the scan's answer that synth.knn does not return, tie-aware: an id at the scan's k-th distance may be swapped for another at that distance"""
    bad = 0
    for i in range(scan_ids.shape[0]):
        absent = ~np.isin(scan_ids[i].astype(np.int64), knn_ids[i].astype(np.int64))
        bad += int((absent & (scan_d[:, i] != scan_d[-1, i])).sum())
    return bad


def walk(e, q, k, L):
    Q = q.shape[0]
    e.set_searchparams(k, L)
    e.alloc(Q)
    out = {}

    def run():
        e.init(Q)
        out["ids"] = e.query(q)[0]
    ms = median_ms(run)
    e.free()
    return ms, out["ids"]


def one(name, log):
    import torch
    rows = []
    ix, q_all, _, _ = exact_sweep.workload(name, 10000, None, log)
    N, D = int(ix.N), int(ix.D)
    dev_vec = torch.from_numpy(ix.vectors()).cuda()
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, distance=bang_amd.DISTANCE_EXACT) as e:
        e.load_index(ix)
        for Q in (100, 10000):
            q = np.ascontiguousarray(q_all[:Q])
            dev_q = torch.from_numpy(q).cuda()
            for k in (10, 100):
                res = {}

                def scan():
                    res["scan"] = e.scan(q, k)
                    res["t"] = e.scan_times()

                def knn():
                    i, d = synth.knn(dev_vec, dev_q, k)
                    res["knn"] = i.cpu().numpy()
                ms_scan, ms_knn = alternate_ms([scan, knn])
                ids, d, _ = res["scan"]
                row = dict(workload=name, Q=Q, k=k, scan_ms=round(ms_scan, 3), scan_launch_ms=round(res["t"]["scan"], 3), merge_ms=round(res["t"]["merge"], 3),
                           knn_ms=round(ms_knn, 3), knn_ids_missed=missed(ids, d, res["knn"]), results=Q * k)
                if ix.dtype != "float":
                    row["i8_mfma_share"] = round(2.0 * N * Q * D / (res["t"]["scan"] * 1e-3) / I8_PEAK_OPS, 4)
                log(json.dumps(row))
                rows.append(row)
        # the exact-distance walk at the smallest L reaching 90 % against the scan, Q = 10 000, k = 10
        q = np.ascontiguousarray(q_all[:10000])
        truth = e.scan(q, 10)
        gt_i, gt_d = (truth[0] & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(truth[1].T)
        for L in WALK_LS:
            ms, ids = walk(e, q, 10, L)
            rec = O.recall(gt_i, gt_d, ids, 10)
            if rec >= 90.0 or L == WALK_LS[-1]:
                row = dict(workload=name, Q=10000, k=10, walk_L=L, walk_ms=round(ms, 3), walk_recall=round(rec, 2))
                log(json.dumps(row))
                rows.append(row)
                break
        # label shares: the scan beside the filtered walk at L = 94, Q = 1 000
        q = np.ascontiguousarray(q_all[:1000])
        labels = labels_sweep.label_table(N, SHARES)
        e.set_labels(labels)
        for b, s in enumerate(SHARES):
            filt = (np.full(1000, 1 << b, np.uint32), np.zeros(1000, np.uint32))
            res = {}

            def scan_f():
                res["scan"] = e.scan(q, 10, *filt)
            e.set_searchparams(10, 94)
            e.alloc(1000)
            e.set_filters(*filt)

            def walk_f():
                e.init(1000)
                res["walk"] = e.query(q)[0]
            ms_scan, ms_walk = alternate_ms([scan_f, walk_f])
            e.free()
            ids, d, matched = res["scan"]
            wids = res["walk"]
            rec = O.recall((ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(d.T), wids, 10)
            row = dict(workload=name, Q=1000, k=10, share=s, scan_ms=round(ms_scan, 3), matched_mean=round(float(matched.mean()), 1), walk_L=94,
                       walk_ms=round(ms_walk, 3), walk_recall_vs_scan=round(rec, 2))
            log(json.dumps(row))
            rows.append(row)
        e.unload()
    return rows


def markdown(rows, commit):
    out = [f"# Exact scan (tools/scan_sweep.py)", "",
           f"Commit {commit}, {datetime.date.today().isoformat()}, one MI355X, one process, contenders alternated, one warm-up and the median of {RUNS} runs.  "
           "Times are host wall time of the whole call in ms (scan launches / merge: GPU time between events).", "",
           "## Scan against synth.knn", "",
           "| workload | Q | k | scan ms | scan launches ms | merge ms | synth.knn ms | knn ids missed (tie-aware) | share of the i8 MFMA rate |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if "knn_ms" in r:
            out.append(f"| {r['workload']} | {r['Q']} | {r['k']} | {r['scan_ms']} | {r['scan_launch_ms']} | {r['merge_ms']} | {r['knn_ms']} | "
                       f"{r['knn_ids_missed']} of {r['results']} | {r.get('i8_mfma_share', '-')} |")
    out += ["", "## The exact-distance walk at the smallest L reaching 90 % 10-recall@10 against the scan (Q = 10 000)", "",
            "| workload | L | walk ms | recall % |", "|---|---|---|---|"]
    for r in rows:
        if "walk_recall" in r:
            out.append(f"| {r['workload']} | {r['walk_L']} | {r['walk_ms']} | {r['walk_recall']} |")
    out += ["", "## Label filters (Q = 1 000, k = 10): the scan beside the filtered walk at L = 94", "",
            "| workload | share % | matched (mean) | scan ms | walk ms | walk recall against the scan % |", "|---|---|---|---|---|---|"]
    for r in rows:
        if "share" in r:
            out.append(f"| {r['workload']} | {r['share']} | {r['matched_mean']} | {r['scan_ms']} | {r['walk_ms']} | {r['walk_recall_vs_scan']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--commit", default=None, help="the commit the tables are headed with (default: git rev-parse of this tree)")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)      # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("scan_sweep needs a HIP device")
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "(no git)"
    except OSError:
        commit = "(no git)"
    rows = []
    for name in a.workloads.split(","):                   # the files are rewritten behind every workload: a run cut short keeps what it has
        rows += one(name, log)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        with open(a.out, "w") as f:
            f.write(markdown(rows, commit))
    log(f"wrote {a.out}")


if __name__ == "__main__":
    main()
