#!/usr/bin/env python3
"""Padded rows (option rows_pad) on the flagship workload, one library per process (BANG_AMD_LIB picks another build): ONE workload build, then REPS x [variants] engine loads, each measured with
bench.measure() at several batch sizes.  Variants are BANG_ROWS_PAD values ("-" = unset).  Prints one JSON line per cell and writes them all to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # tools/ -> the repository
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--variants", default="-")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", default="10000,2500,1250")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape-n", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import bench
    import bang_amd
    from oracle import oracle as O  # noqa: F401
    ctx = bench.Ctx()
    ctx.rank, ctx.local_rank, ctx.world, ctx.k, ctx.weak, ctx.live_traffic = 0, 0, 1, 10, False, None
    torch.cuda.set_device(0)
    ctx.dev = ctx.cdev = torch.device("cuda", 0)
    qs = [int(x) for x in a.queries.split(",")]
    t0 = time.time()
    wl = bench.build_workload("sift1b_shape", ctx, Q=max(qs), shape_n=a.shape_n, stream=True)
    print(f"[ab] workload in {time.time() - t0:.0f}s", flush=True)
    L = 152
    rows, ref = [], {}
    for rep in range(a.reps):
        for var in a.variants.split(","):
            if var == "-":
                os.environ.pop("BANG_ROWS_PAD", None)
            else:
                os.environ["BANG_ROWS_PAD"] = var
            t0 = time.time()
            eng = bench.make_engine(wl, wl["graph"], ctx, timing=1)
            t_load = time.time() - t0
            n_pad = eng.rows_pad() if hasattr(eng, "rows_pad") and hasattr(bang_amd.lib(), "bang_rows_pad_e") else 0
            for q in qs:
                my_q = np.ascontiguousarray(wl["queries"][:q])
                ctx.Q_total = q
                eng.set_searchparams(ctx.k, L)
                eng.alloc(q)
                res = bench.measure(eng, wl, my_q, L, a.steps, a.warmup, ctx, wl["graph"])
                st = res["agg"]
                same = None
                if q in ref:
                    same = bool(np.array_equal(ref[q][0], res["ids"]) and np.array_equal(ref[q][1].view(np.uint32), res["dists"].view(np.uint32)))
                else:
                    ref[q] = (res["ids"].copy(), res["dists"].copy())
                eng.free()
                r = res["roofline"] or {}
                rows.append(dict(tag=a.tag, rep=rep, rows_pad=var, queries=q, ms=res["ms_per_step"], launch_us=r.get("avg_launch_us"), n_pad=n_pad,
                                 rows_in_hbm=int(st["rows_in_hbm"]), own_hbm_per_step=int(st["rows_from_own_hbm"]) // a.steps,
                                 pulled_bytes_per_step=int(st["pulled_bytes"]) // a.steps, iterations=int(st["iterations"]),
                                 dist_evals=int(st["dist_evals"]), load_s=round(t_load, 1), step_ms=res["step_ms"], same_ids_as_first=same,
                                 ids_crc=int(np.bitwise_xor.reduce(res["ids"].astype(np.uint64).ravel())), dists_crc=int(np.bitwise_xor.reduce(res["dists"].view(np.uint32).ravel()))))
                print(json.dumps(rows[-1]), flush=True)
            eng.unload()
            eng.close()
    wl["release"]()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
