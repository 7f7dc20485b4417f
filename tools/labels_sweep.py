#!/usr/bin/env python3
"""What per-query label filters (Engine.set_labels / set_filters) cost and what they return, on the SAME load of the SAME index in
the SAME process.  Exact-distance mode (distance = 1); every query of a batch carries the same filter here, so that the post-filter composition --
the exclusion of the complement, Engine.set_excluded, DESIGN.md 4.12 -- can stand beside it.  Columns per L:

  unfiltered        labels loaded, no filters: the plain exact-distance launch -- the time base
  filtered s %      any = one label bit that s per cent of the points carry: bang_k_search_exact_labels, results collected during the walk
  post-filter s %   no filters; the complement of that bit excluded: the plain launch at rr_k = L + bang_k_worklist_pick on the final worklist

Workloads (tools/exact_sweep.py): structured synthetic 10^6-point indexes, SIFT1M-like (uint8, D = 128) and DEEP-like (float, D = 96).  Per
workload, placement, L and column: one warm-up bang_query and --runs timed ones (bang_init outside the timed region); ms per batch (best and
median: host wall time of bang_query), 10-recall@10 against the FILTERED brute-force truth (synth.knn over the matching points only), the mean
matched count and the padded result slots.  The columns alternate per L, so all see the same clocks.  Registers and waves per CU of the new
instances are read from the code objects.  There is no threshold: the numbers are a record.

  python tools/labels_sweep.py --workloads sift1m,deep1m --out profiles/labels_sweep.json --md profiles/labels_sweep.md

Not part of bench.py: the measurement behind profiles/labels.md.
"""
import argparse
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
from oracle import oracle as O  # noqa: E402
import exact_sweep  # noqa: E402
import exclude_sweep  # noqa: E402

SEED = 20261


def label_table(N, shares):
    """bit b set on shares[b] per cent of the points, independently, fixed seed"""
    rng = np.random.default_rng(SEED)
    lab = np.zeros(N, np.uint32)
    for b, s in enumerate(shares):
        lab |= (rng.random(N) < s / 100.0).astype(np.uint32) << np.uint32(b)
    return lab


def instance_registers():
    """{kernel: [(dtype code, VGPRs, scratch bytes, waves per CU by registers)]} of the two label-filter code objects, or {} without llvm binutils"""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        return {}
    out = {}
    for obj, kernel in (("bang_search_exact_labels.o", "search_exact_labels_kernel"), ("bang_search_exact_labels_pull.o", "search_exact_labels_pull_kernel")):
        path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", obj)
        if not os.path.exists(path):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
            subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "unused.o")], check=True)
            subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
            notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in notes.split(".name:")[1:]:
            m = re.match(r"_Z\d+" + kernel + r"ILi(\d)EEv9ExactArgs$", blk.split()[0])
            if m:
                vg = int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1))
                sc = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
                out.setdefault(kernel, []).append((int(m.group(1)), vg, sc, 4 * min(8, 512 // ((vg + 7) & ~7))))
    return out


def measure(e, workload, placement, ix, q, labels, shares, truth, Ls, k, runs, log):
    rows = []
    Q = q.shape[0]
    N = int(ix.N)
    cols = [("unfiltered", None, None)]
    for b, s in enumerate(shares):
        cols += [(f"filtered {s:g} %", b, "filter"), (f"post-filter {s:g} %", b, "exclude")]
    e.set_labels(labels)
    for L in Ls:
        for name, bit, how in cols:
            if how == "exclude":
                e.set_excluded(np.nonzero((labels >> np.uint32(bit)) & 1 == 0)[0].astype(np.uint32))
            else:
                e.clear_excluded()
            e.set_searchparams(k, L)
            e.alloc(Q)
            if how == "filter":
                e.set_filters(np.full(Q, 1 << bit, np.uint32), np.zeros(Q, np.uint32))
            times, ids = [], None
            for r in range(runs + 1):                         # run 0: warm-up
                e.init(Q)
                t0 = time.perf_counter()
                ids, _ = e.query(q)
                dt = time.perf_counter() - t0
                if r:
                    times.append(dt)
            st = e.query_counters(Q)
            s = e.stats()
            matched = e.matched_counts(Q) if how == "filter" else None
            e.free()
            assert int(s["label_launches"]) == (1 if how == "filter" else 0) and int(s["exclude_launches"]) == (1 if how == "exclude" else 0), s
            gt = truth.get(bit)
            row = {"workload": workload, "placement": placement, "column": name, "share": shares[bit] if bit is not None else 100, "how": how or "none",
                   "Q": Q, "L": L, "recall": round(O.recall(gt[0][:Q], gt[1][:Q], ids, k), 3) if gt is not None else None,
                   "ms_best": round(1e3 * min(times), 4), "ms_median": round(1e3 * float(np.median(times)), 4),
                   "evals": round(float(st[:, 2].mean()), 2), "matched_mean": round(float(matched.mean()), 2) if matched is not None else None,
                   "padded": int((ids == np.iinfo(np.uint64).max).sum())}
            log(json.dumps(row))
            rows.append(row)
    e.clear_excluded()
    return rows


def markdown(out):
    s = []
    if out["registers"]:
        s += ["| kernel | dtype | VGPRs | scratch bytes | waves per CU (registers) |", "|---|---|---|---|---|"]
        for kname, inst in out["registers"].items():
            for dt, vg, sc, waves in sorted(inst):
                s.append(f"| {kname} | {('u8', 'i8', 'f32')[dt]} | {vg} | {sc} | {waves} |")
        s.append("")
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']}, D = {w['D']}, {w['dtype']}, R = {w['R']}; k = {out['k']}, {out['runs']} timed runs per point; "
              f"points matching: {', '.join(f'{a:g} % asked, {b:.2f} % drawn' for a, b in zip(out['shares'], w['drawn']))}", ""]
        for placement in sorted({r["placement"] for r in out["rows"] if r["workload"] == w["name"]}):
            sel = [r for r in out["rows"] if r["workload"] == w["name"] and r["placement"] == placement]
            note = "graph = device" if placement == "device" else "graph = host (pull = 1, every row over PCIe)"
            s += [f"{note}, {sel[0]['Q']} queries", "",
                  "| L | column | ms (best) | ms (median) | time / unfiltered | 10-recall@10 (filtered truth) | matched per query | padded slots |", "|---|---|---|---|---|---|---|---|"]
            base = {r["L"]: r["ms_best"] for r in sel if r["column"] == "unfiltered"}
            for r in sel:
                rec = f"{r['recall']:.2f}" if r["recall"] is not None else "not measured"
                mt = f"{r['matched_mean']:.1f}" if r["matched_mean"] is not None else "-"
                s.append(f"| {r['L']} | {r['column']} | {r['ms_best']:.3f} | {r['ms_median']:.3f} | {r['ms_best'] / base[r['L']]:.3f} | {rec} | {mt} | {r['padded']} |")
            s.append("")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--placements", default="device")
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--shares", default="50,10,1", help="per cent of the points that carry label bit 0, 1, ...")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cache", default="", help="directory of index prefixes to write / reuse (as tools/exact_sweep.py)")
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("labels_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")]
    shares = [float(x) for x in a.shares.split(",") if x]
    out = {"k": k, "runs": a.runs, "shares": shares, "registers": instance_registers(), "workloads": [], "rows": []}

    def flush():
        for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)

    for name in a.workloads.split(","):
        ix, q, gi, gd = exact_sweep.workload(name, a.batch, os.path.join(a.cache, name) if a.cache else "", log)
        q = np.ascontiguousarray(q[:a.batch])
        labels = label_table(int(ix.N), shares)
        t0 = time.time()
        dev = torch.device("cuda", 0)
        x = torch.from_numpy(ix.vectors().astype(np.float32)).to(dev)
        qq = torch.from_numpy(q.astype(np.float32)).to(dev)
        truth = {None: (np.ascontiguousarray(gi[:a.batch], dtype=np.uint32), np.ascontiguousarray(gd[:a.batch], dtype=np.float32))}
        for b in range(len(shares)):
            truth[b] = exclude_sweep.live_truth(x, qq, np.nonzero((labels >> np.uint32(b)) & 1 == 0)[0].astype(np.uint32), k)
        del x, qq
        torch.cuda.empty_cache()
        log(f"filtered brute-force truth for {shares} %: {time.time() - t0:.1f} s")
        out["workloads"].append({"name": name, "N": int(ix.N), "D": int(ix.D), "dtype": ix.dtype, "m": int(ix.m), "R": int(ix.R),
                                 "drawn": [100.0 * float(((labels >> np.uint32(b)) & 1).mean()) for b in range(len(shares))]})
        for placement in a.placements.split(","):
            opts = dict(graph=bang_amd.GRAPH_DEVICE) if placement == "device" else dict(graph=bang_amd.GRAPH_HOST, pull=1, rows_hbm=0)
            with bang_amd.Engine(ix.dtype, distance=1, **opts) as e:
                e.load_index(ix)
                out["rows"] += measure(e, name, placement, ix, q, labels, shares, truth, Ls, k, a.runs, log)
                e.unload()
            flush()
        del ix
    flush()


if __name__ == "__main__":
    main()
