#!/usr/bin/env python3
"""What inserts (option capacity, Engine.insert) cost and what they do to recall.  Graph in HBM.

Workloads (the shapes of tools/exact_sweep.py): structured synthetic 10^6-point indexes, SIFT1M-like (uint8, D = 128, m = 32) and DEEP-like (float,
D = 96, m = 74), R = 64.  Per workload one set of N vectors, Q queries and their brute-force 10-NN over all N, and two indexes built by
bang_amd.synth: FULL over all N points, and PART over the first 90 % -- the remaining 10 % are inserted into PART.
The builder is synth.build_graph / synth.train_pq (brute-force kNN graph, the builder of tools/exact_sweep.py and tools/range_sweep.py at this N),
NOT bang_amd.index_build: make_index_large generates its own vectors from N and a seed, so it cannot build PART over a given nine tenths of the
vectors FULL is built over, and its partitioned candidate search is written for N of a few million and more.  The recall columns therefore sit
beside those of profiles/exact_distance.md and profiles/range_search.md (same builder), not beside bench.py's Vamana-style indexes.

  throughput   batches of 256 and 4096 points at L_build 64 and 128 (alpha 1.2), --batches of each: points/s from the host wall time of
               Engine.insert, and the share of the candidate search, the prune of the new rows, the back-edge launches, the PQ encode (stream time
               between event stamps) and the host-side part (new rows down + grouping by target) in the call (bang_get_insert_times).  The points
               these batches insert are part of the 10 %; the rest follows in batches of 4096 at L_build 64.
  recall       10-recall@10 over the L grid on the exact walk (distance = 1) and on the self-paced PQ walk, PART + inserts against FULL.
  registers    VGPRs, scratch and LDS of the new kernels, read from the code object.

There is no threshold: the parent cannot insert, the numbers are the baseline for later work.

  python tools/insert_sweep.py --workloads sift1m,deep1m --out profiles/insert.json --md profiles/insert.md
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

import bang_amd  # noqa: E402
from bang_amd import formats, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

WORKLOADS = {
    "sift1m": (1_000_000, 128, "uint8", 64, 32, 256),
    "deep1m": (1_000_000, 96, "float", 64, 74, 256),
    "small": (100_000, 128, "uint8", 64, 32, 64),
}
KERNELS = ("prune_kernel", "backedge_kernel", "pq_argmin_kernel", "worklist_lists_kernel")
PRUNE_WAVE_BYTES = 4 * (2 * 512 + 16 + 64 + 3 * 512)          # PRUNE_WAVE_WORDS of csrc/bang_insert.hip: dynamic LDS per wave


def kernel_resources():
    """[(kernel, VGPRs, scratch bytes, static LDS bytes)] of lib/bang_insert.o, or [] without llvm binutils / the object"""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_insert.o")
    if not all(os.path.exists(t) for t in tools) or not os.path.exists(path):
        return []
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, os.path.join(tmp, "unused.o")], check=True)
        subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
        notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    out = []
    for blk in notes.split("- .agpr_count:")[1:]:                       # one block per kernel: .agpr_count is the first key of its map
        nm = re.search(r"\.name:\s*(\S+)", blk)
        name = nm.group(1) if nm else ""
        k = next((k for k in KERNELS if k in name), None)
        if not k:
            continue
        m = re.search(r"ILi(\d)E", name)
        inst = ("u8", "i8", "f32")[int(m.group(1))] if m else "-"
        get = lambda key: int(re.search(key + r":\s*(\d+)", blk).group(1))     # noqa: E731
        out.append((k, inst, get(r"\.vgpr_count"), get(r"\.private_segment_fixed_size"), get(r"\.group_segment_fixed_size")))
    return sorted(set(out))


def build(x, dtype, R, m, seed, log, what):
    """formats.Index over the rows of x (a tensor on the build device): synth.make_index's steps on vectors that exist already"""
    t0 = time.time()
    deg, adj = synth.build_graph(x, R, seed=seed)
    medoid = int(synth._sq_norms(x - x.mean(dim=0)).argmin())
    pivots, centroid, off, codes = synth.train_pq(x, m, seed=seed)
    graph = formats.pack_graph(synth.to_numpy(x, dtype), deg.cpu().numpy().astype(np.uint32), adj.cpu().numpy().astype(np.uint32))
    log(f"built {what}: N = {x.shape[0]} in {time.time() - t0:.1f} s")
    return formats.Index(dtype=dtype, N=int(x.shape[0]), D=int(x.shape[1]), R=R, m=m, medoid=medoid, graph=graph, codes=codes.cpu().numpy(),
                         pivots=pivots.cpu().numpy().astype(np.float32), centroid=centroid.cpu().numpy().astype(np.float32), chunk_off=off)


def recall_rows(e, workload, index_name, q, gi, gd, Ls, k, log):
    rows = []
    Q = q.shape[0]
    for mode, distance in (("exact", 1), ("pq", 0)):
        e.set_option("distance", distance)
        e.set_option("search", 1)
        for L in Ls:
            e.set_searchparams(k, L)
            e.alloc(Q)
            e.init(Q)
            ids, _ = e.query(q)
            e.free()
            row = {"workload": workload, "index": index_name, "walk": mode, "L": L, "recall": round(O.recall(gi, gd, ids, k), 3)}
            log(json.dumps(row))
            rows.append(row)
    return rows


def markdown(out):
    s = []
    if out["resources"]:
        s += ["| kernel | instance | VGPRs | scratch bytes | static LDS bytes | dynamic LDS per wave |", "|---|---|---|---|---|---|"]
        for k, inst, vg, sc, lds in out["resources"]:
            s.append(f"| {k} | {inst} | {vg} | {sc} | {lds} | {PRUNE_WAVE_BYTES if k == 'prune_kernel' else 0} |")
        s.append("")
    for w in out["workloads"]:
        s += [f"### {w['name']}: N = {w['N']} ({w['N_part']} indexed + {w['N'] - w['N_part']} inserted), D = {w['D']}, {w['dtype']}, R = {w['R']}, m = {w['m']}; "
              f"alpha = {out['alpha']}; back-edge rows appended / pruned / incoming ids dropped: {w['appended']} / {w['pruned']} / {w['dropped']}", ""]
        s += ["| batch | L_build | batches | points/s (best) | points/s (median) | search % | prune % | back-edges % | encode % | host grouping % | other % |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in [r for r in out["throughput"] if r["workload"] == w["name"]]:
            sh = r["share"]
            s.append(f"| {r['batch']} | {r['L_build']} | {r['batches']} | {r['pps_best']:.0f} | {r['pps_median']:.0f} | {sh['search']:.1f} | {sh['prune']:.1f} | "
                     f"{sh['backedge']:.1f} | {sh['encode']:.1f} | {sh['group']:.1f} | {sh['other']:.1f} |")
        s += ["", "| walk | L | 10-recall@10, 90 % built + 10 % inserted | 10-recall@10, built over all points |", "|---|---|---|---|"]
        rec = {(r["index"], r["walk"], r["L"]): r["recall"] for r in out["recall"] if r["workload"] == w["name"]}
        for walk in ("exact", "pq"):
            for L in out["Ls"]:
                if ("inserted", walk, L) in rec:
                    s.append(f"| {walk} | {L} | {rec[('inserted', walk, L)]:.2f} | {rec.get(('full', walk, L), float('nan')):.2f} |")
        s.append("")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--batches", type=int, default=2, help="timed batches per (batch size, L_build)")
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("insert_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")]
    out = {"k": k, "alpha": a.alpha, "Ls": Ls, "resources": kernel_resources(), "workloads": [], "throughput": [], "recall": []}

    def flush():
        for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)

    for name in a.workloads.split(","):
        N, D, dtype, R, m, ncl = WORKLOADS[name]
        seed = synth.SEED
        x = synth.make_vectors(N, D, dtype, n_clusters=ncl, seed=seed, device="cuda")
        x = x[torch.randperm(N, generator=torch.Generator().manual_seed(seed)).to(x.device)]     # (the inserted tenth is a random tenth)
        qt = synth.make_queries(x, a.queries, dtype, seed=seed)
        gi, gd = synth.knn(x, qt, k)
        q, gi, gd = np.ascontiguousarray(synth.to_numpy(qt, dtype)), gi.cpu().numpy().astype(np.uint32), gd.cpu().numpy().astype(np.float32)
        Np = N - N // 10
        full = build(x, dtype, R, m, seed, log, f"{name} full")
        part = build(x[:Np], dtype, R, m, seed, log, f"{name} part")
        new = np.ascontiguousarray(synth.to_numpy(x[Np:], dtype))
        del x, qt
        torch.cuda.empty_cache()
        with bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE) as e:
            e.load_index(full)
            out["recall"] += recall_rows(e, name, "full", q, gi, gd, Ls, k, log)
        del full
        with bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE, capacity=N) as e:
            e.load_index(part)
            at = 0
            for batch, Lb in ((256, 64), (4096, 64), (256, 128), (4096, 128)):
                pps, shares = [], []
                for _ in range(a.batches):
                    v = new[at:at + batch]
                    at += batch
                    t0 = time.perf_counter()
                    e.insert(v, Lb, a.alpha)
                    pps.append(batch / (time.perf_counter() - t0))
                    t = e.insert_times()
                    shares.append({p: 100.0 * t[p] / t["total"] for p in ("search", "prune", "group", "backedge", "encode")})
                share = {p: float(np.mean([s[p] for s in shares])) for p in shares[0]}
                share["other"] = 100.0 - sum(share.values())            # allocations, the vector and entry uploads, the seed list
                row = {"workload": name, "batch": batch, "L_build": Lb, "batches": a.batches, "pps_best": max(pps), "pps_median": float(np.median(pps)),
                       "share": share}
                log(json.dumps(row))
                out["throughput"].append(row)
            t0 = time.time()
            while at < len(new):
                e.insert(new[at:at + 4096], 64, a.alpha)
                at += 4096
            log(f"the rest of the {len(new)} points inserted in {time.time() - t0:.1f} s")
            assert e.num_nodes() == N
            st = e.insert_stats()
            out["workloads"].append({"name": name, "N": N, "N_part": Np, "D": D, "dtype": dtype, "R": R, "m": m, "appended": st["backedge_appended"],
                                     "pruned": st["backedge_pruned"], "dropped": st["backedge_dropped"]})
            out["recall"] += recall_rows(e, name, "inserted", q, gi, gd, Ls, k, log)
        flush()
        del part, new
    flush()


if __name__ == "__main__":
    main()
