#!/usr/bin/env python3
"""What range search (option range_hits, Engine.set_radii) costs and what it returns, on the SAME load of the SAME index in the SAME
process.  Exact-distance mode (distance = 1), graph in HBM.  Columns per L:

  plain             range_hits set, no radii: the plain exact-distance launch (the parent commit's kernel, device code unchanged) -- the time base
  radius -1         every query's radius -1: bang_k_search_exact_range + bang_k_range_sort, nothing within range -- what the hit test alone costs
  rank N            every query's radius the brute-force distance of its rank-N point, N = 10 / 100 / 1000 (float vectors: times 1 + 1e-5, so that
                    the rank-N point itself is inside whatever the two arithmetics round)

Workloads (tools/exact_sweep.py): structured synthetic 10^6-point indexes, SIFT1M-like (uint8, D = 128) and DEEP-like (float, D = 96).  Per
workload, L and column: one warm-up bang_query and --runs timed ones (bang_init outside the timed region); ms per batch (best and median: host
wall time of bang_query, the sort launch included), RANGE RECALL = the share of a query's brute-force rank-N points that are among its hits
(mean over the batch), hits and offered per query, truncated queries.  The columns alternate per L, so all see the same clocks.  The sort kernel
alone: bang_k_range_sort on rows of random keys with the batch's own offered counts, host wall time of launch + synchronise.  Registers and waves
per CU of the new instances are read from the code objects.  There is no threshold: the numbers are a record.

  python tools/range_sweep.py --workloads sift1m,deep1m --out profiles/range_sweep.json --md profiles/range_sweep.md

Not part of bench.py: the measurement behind profiles/range_search.md.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bang_amd  # noqa: E402
from bang_amd import binding as B  # noqa: E402
from bang_amd import synth  # noqa: E402
import exact_sweep  # noqa: E402

RANKS = (10, 100, 1000)
OBJECTS = (("bang_search_exact_range.o", "search_exact_range_kernel"), ("bang_search_exact_range_pull.o", "search_exact_range_pull_kernel"),
           ("bang_range.o", "range_sort_kernel"))


def instance_registers():
    """{kernel: [(instance, VGPRs, scratch bytes, waves per CU by registers)]} of the new code objects, or {} without llvm binutils"""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        return {}
    out = {}
    for obj, kernel in OBJECTS:
        path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", obj)
        if not os.path.exists(path):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
            subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "unused.o")], check=True)
            subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
            notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in notes.split(".name:")[1:]:
            m = re.match(r"_Z\d+" + kernel + r"(?:ILi(\d)EEv9ExactArgs|\d+RangeSortArgs)$", blk.split()[0])
            if m:
                vg = int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1))
                sc = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
                out.setdefault(kernel, []).append((("u8", "i8", "f32")[int(m.group(1))] if m.group(1) else "-", vg, sc, 4 * min(8, 512 // ((vg + 7) & ~7))))
    return out


def sort_alone(offered, cap, reps):
    """bang_k_range_sort on [Q][cap] rows of random keys with these offered counts: ms per launch (best, median), launch + synchronise"""
    Q = len(offered)
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 1 << 20, (Q, cap), dtype=np.uint32)
    d = rng.integers(0, 1 << 16, (Q, cap)).astype(np.float32)
    bufs = [B.DeviceBuffer.from_numpy(x) for x in (ids, d, np.ascontiguousarray(offered, np.uint32), np.zeros(Q, np.uint32))]
    f = B.lib().bang_k_range_sort
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    times = []
    try:
        for r in range(reps + 1):                                 # (a sorted row is sorted again: the network does the same work)
            B.sync()
            t0 = time.perf_counter()
            rc = f(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, cap, 0, Q, Q, bufs[3].ptr, None)
            B.sync()
            if rc != 0:
                raise RuntimeError(B.lib().bang_last_error().decode())
            if r:
                times.append(time.perf_counter() - t0)
    finally:
        for b in bufs:
            b.free()
    return round(1e3 * min(times), 4), round(1e3 * float(np.median(times)), 4)


def measure(e, workload, ix, q, truth_ids, radii, Ls, k, cap, runs, log):
    rows = []
    Q = q.shape[0]
    cols = [("plain", None), ("radius -1", np.full(Q, -1.0, np.float32))] + [(f"rank {n}", radii[n]) for n in RANKS]
    for L in Ls:
        for name, r in cols:
            e.set_searchparams(k, L)
            e.alloc(Q)
            if r is not None:
                e.set_radii(r)
            times = []
            for i in range(runs + 1):                             # run 0: warm-up
                e.init(Q)
                t0 = time.perf_counter()
                e.query(q)
                dt = time.perf_counter() - t0
                if i:
                    times.append(dt)
            st = e.query_counters(Q)
            s = e.stats()
            row = {"workload": workload, "column": name, "Q": Q, "L": L, "cap": cap, "ms_best": round(1e3 * min(times), 4),
                   "ms_median": round(1e3 * float(np.median(times)), 4), "evals": round(float(st[:, 2].mean()), 2), "recall": None, "hits": None,
                   "offered": None, "truncated": int(s["range_truncated"]), "sort_ms_best": None, "sort_ms_median": None}
            assert int(s["range_launches"]) == (0 if r is None else 1) and int(s["front_launches"]) == 1, s
            if r is not None:
                counts, offered = e.range_counts(Q)
                lims, ids, _ = e.range_results(Q)
                row["hits"], row["offered"] = round(float(counts.mean()), 2), round(float(offered.mean()), 2)
                if name.startswith("rank"):
                    n = int(name.split()[1])
                    found = 0
                    for i in range(Q):
                        found += np.intersect1d(ids[int(lims[i]):int(lims[i + 1])], truth_ids[i, :n], assume_unique=True).size
                    row["recall"] = round(100.0 * found / (Q * n), 3)
                row["sort_ms_best"], row["sort_ms_median"] = sort_alone(offered, cap, runs)
            e.free()
            log(json.dumps(row))
            rows.append(row)
    return rows


def markdown(out):
    s = []
    if out["registers"]:
        s += ["| kernel | instance | VGPRs | scratch bytes | waves per CU (registers) |", "|---|---|---|---|---|"]
        for kname, inst in out["registers"].items():
            for dt, vg, sc, waves in sorted(inst):
                s.append(f"| {kname} | {dt} | {vg} | {sc} | {waves} |")
        s.append("")
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']}, D = {w['D']}, {w['dtype']}, R = {w['R']}; graph = device; k = {out['k']}, range_hits = {out['cap']}, "
              f"{out['runs']} timed runs per point; mean radius at rank 10 / 100 / 1000: {' / '.join(f'{x:.4g}' for x in w['radius_mean'])}", ""]
        sel = [r for r in out["rows"] if r["workload"] == w["name"]]
        if not sel:
            continue
        s += [f"{sel[0]['Q']} queries", "",
              "| L | column | ms (best) | ms (median) | time / plain | range recall % | hits per query | offered per query | truncated queries | sort alone ms (best) |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        base = {r["L"]: r["ms_best"] for r in sel if r["column"] == "plain"}
        for r in sel:
            f = lambda v, fmt="{:.2f}": fmt.format(v) if v is not None else "-"      # noqa: E731
            s.append(f"| {r['L']} | {r['column']} | {r['ms_best']:.3f} | {r['ms_median']:.3f} | {r['ms_best'] / base[r['L']]:.3f} | {f(r['recall'])} | "
                     f"{f(r['hits'], '{:.1f}')} | {f(r['offered'], '{:.1f}')} | {r['truncated']} | {f(r['sort_ms_best'], '{:.3f}')} |")
        s.append("")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--cap", type=int, default=2048, help="option range_hits")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cache", default="", help="directory of index prefixes to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("range_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")]
    out = {"k": k, "runs": a.runs, "cap": a.cap, "registers": instance_registers(), "workloads": [], "rows": []}

    def flush():
        for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)

    for name in a.workloads.split(","):
        ix, q, _, _ = exact_sweep.workload(name, a.batch, os.path.join(a.cache, name) if a.cache else "", log)
        q = np.ascontiguousarray(q[:a.batch])
        t0 = time.time()
        dev = torch.device("cuda", 0)
        x = torch.from_numpy(ix.vectors().astype(np.float32)).to(dev)
        qq = torch.from_numpy(q.astype(np.float32)).to(dev)
        ti, td = synth.knn(x, qq, max(RANKS))
        truth_ids = ti.cpu().numpy().astype(np.uint64)
        td = td.cpu().numpy().astype(np.float32)
        del x, qq, ti
        torch.cuda.empty_cache()
        slack = np.float32(1.0 + 1e-5) if ix.dtype == "float" else np.float32(1.0)
        radii = {n: np.ascontiguousarray(td[:, n - 1] * slack, np.float32) for n in RANKS}
        log(f"brute-force truth to rank {max(RANKS)}: {time.time() - t0:.1f} s")
        out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R),
                                 "radius_mean": [float(radii[n].mean()) for n in RANKS]})
        with bang_amd.Engine(ix.dtype, distance=1, graph=bang_amd.GRAPH_DEVICE, range_hits=a.cap) as e:
            e.load_index(ix)
            out["rows"] += measure(e, name, ix, q, truth_ids, radii, Ls, k, a.cap, a.runs, log)
            e.unload()
        flush()
        del ix
    flush()


if __name__ == "__main__":
    main()
