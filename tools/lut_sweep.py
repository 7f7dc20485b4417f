#!/usr/bin/env python3
"""The PQ walk of LUT-path indexes, graph in HBM: the query-resident kernel (search = 1, bang_k_search_lut) against the launch-per-iteration
loop (search = -1, what these layouts ran before and still run by default), on GIST-like (float, D = 960, m = 120) and MNIST-like (uint8,
D = 784, m = 98) structured synthetic indexes (bang_amd.synth, as tools/exact_highdim.py builds them).

Per layout, on ONE build of the index (an engine per mode, both loaded for the whole step): both modes over the L grid (recall, queries/s); then --runs timed batches per mode, the modes
ALTERNATING, at each mode's smallest L with 10-recall@10 >= --target (the walk is the same in both modes, so the two L agree).  Reported per
mode: queries/s median, best, worst; recall.  The bar: the kernel's median queries/s exceeds the loop's median by more than the loop's own
spread (best - worst).  Also recorded: the kernel instance's VGPRs and scratch (hipcc's resource-usage remarks) and its launch geometry.

Every layout is one GPU step: a child process under its own `timeout`; the first step that fails ends the run.

  python tools/lut_sweep.py --n 100000 --out profiles/lut_search.json

Not part of bench.py: the measurement behind profiles/lut_search.md.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bang-billion-scale-ann_amd"))

# name: (D, dtype, m)
LAYOUTS = {"gist_like": (960, "float", 120), "mnist_like": (784, "uint8", 98)}
MODES = {"kernel": 1, "loop": -1}                            # option "search"


def log(s):
    print(s, flush=True)


class Runner:
    """One engine on a loaded index; batch(L) times one bang_query (bang_init outside the timed region)."""
    def __init__(self, bang_amd, ix, q, mode, k):
        self.q, self.Q, self.k, self.L = q, q.shape[0], k, None
        self.e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, search=MODES[mode])
        self.e.load_index(ix)

    def at(self, L):
        if self.L is not None:
            self.e.free()
        self.e.set_searchparams(self.k, L)
        self.e.alloc(self.Q)
        self.L = L
        self.batch()                                          # warm-up

    def batch(self):
        self.e.init(self.Q)
        t0 = time.perf_counter()
        self.ids, _ = self.e.query(self.q)
        return time.perf_counter() - t0

    def close(self):
        if self.L is not None:
            self.e.free()
        self.e.unload()
        self.e.close()


def child(a):
    import bang_amd
    from bang_amd import synth
    from oracle import oracle as O
    D, dtype, m = LAYOUTS[a.child]
    k = 10
    t0 = time.time()
    ix, q, gi, gd = synth.make_index(a.n, D, dtype, a.R, m, a.queries, K=k, n_clusters=64, device="cuda", pq_iters=4)
    log(f"built {a.child}: N={a.n} D={D} {dtype} R={a.R} m={m} Q={a.queries} in {time.time() - t0:.1f} s")
    rec = {"D": D, "dtype": dtype, "m": m, "rows": [], "at_target": {}}
    run = {mode: Runner(bang_amd, ix, q, mode, k) for mode in MODES}
    for L in range(k, a.max_L + 1, a.step_L):
        for mode, r in run.items():                           # the modes alternate at every L
            r.at(L)
            t = r.batch()
            s = r.e.stats()
            assert s["search_kernel"] == (1 if mode == "kernel" else 0), (mode, s["search_kernel"])
            row = {"mode": mode, "L": L, "recall": round(O.recall(gi, gd, r.ids, k), 3), "ms": round(1e3 * t, 3), "qps": round(a.queries / t),
                   "launches": int(s["front_launches"])}
            rec["rows"].append(row)
            log(json.dumps(row))
            if mode not in rec["at_target"] and row["recall"] >= a.target:
                rec["at_target"][mode] = L
        if len(rec["at_target"]) == len(MODES):
            break
    if len(rec["at_target"]) == len(MODES):
        times = {mode: [] for mode in MODES}
        for mode, r in run.items():
            r.at(rec["at_target"][mode])
        for _ in range(a.runs):
            for mode, r in run.items():
                times[mode].append(r.batch())
        alt = {}
        for mode, r in run.items():
            qps = sorted(a.queries / t for t in times[mode])
            alt[mode] = {"L": rec["at_target"][mode], "ms": [round(1e3 * t, 3) for t in times[mode]], "qps_median": round(float(np.median(qps))),
                         "qps_best": round(qps[-1]), "qps_worst": round(qps[0]), "recall": round(O.recall(gi, gd, r.ids, k), 3)}
        same = bool(np.array_equal(run["kernel"].ids, run["loop"].ids)) if alt["kernel"]["L"] == alt["loop"]["L"] else None
        spread = alt["loop"]["qps_best"] - alt["loop"]["qps_worst"]
        rec["alternating"] = dict(alt, same_ids=same, loop_spread_qps=spread, ratio=round(alt["kernel"]["qps_median"] / alt["loop"]["qps_median"], 2),
                                  met=bool(alt["kernel"]["L"] == alt["loop"]["L"] and alt["kernel"]["qps_median"] > alt["loop"]["qps_median"] + spread))
        log(json.dumps({a.child: rec["alternating"]}))
    wg, wv = C.c_uint32(), C.c_uint32()
    L_geo = rec["at_target"].get("kernel", k)
    if bang_amd.lib().bang_search_lut_geometry(C.c_uint32(L_geo), C.c_uint32(a.queries), C.c_uint32(0), C.c_uint32(0), C.byref(wg), C.byref(wv)) == 0:
        rec["geometry"] = {"L": L_geo, "workgroups": wg.value, "waves_per_workgroup": wv.value}
    for r in run.values():
        r.close()
    with open(a.child_out, "w") as f:
        json.dump(rec, f)


def instance_usage():
    """VGPRs / SGPRs / scratch of search_lut_kernel as compiled (no GPU needed), or None where there is no compiler."""
    try:
        from tools.dev import kernel_usage
        src = os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_search_lut.hip")
        rows = kernel_usage.rows(kernel_usage.usage_of(src, ["-fslp-vectorize"]), "search_lut_kernel")     # (the Makefile's flags for this unit)
        r = rows[0]
        alloc = (r["vgpr"] + 7) & ~7
        return {"vgpr": r["vgpr"], "sgpr": r["sgpr"], "scratch_bytes_per_lane": r["scratch"], "waves_per_cu_by_registers": 4 * min(8, 512 // alloc)}
    except (Exception, SystemExit) as ex:                     # noqa: BLE001
        return {"error": str(ex)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--indexes", default="gist_like,mnist_like")
    ap.add_argument("--max-L", type=int, default=130)
    ap.add_argument("--step-L", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--target", type=float, default=90.0)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one layout's GPU step may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"N": a.n, "R": a.R, "Q": a.queries, "k": 10, "runs": a.runs, "target": a.target, "instance": instance_usage(), "indexes": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    dump()
    for name in [x for x in a.indexes.split(",") if x]:
        tmp = (a.out or os.path.join(ROOT, "lut_sweep")) + f".{name}.part"
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--child-out", tmp,
               "--n", str(a.n), "--R", str(a.R), "--queries", str(a.queries), "--max-L", str(a.max_L), "--step-L", str(a.step_L), "--runs", str(a.runs),
               "--target", str(a.target)]
        rc = subprocess.run(cmd).returncode
        if rc != 0 or not os.path.exists(tmp):                # a GPU step that failed or ran out of time: nothing more is started
            out["indexes"][name] = {"error": f"step ended with status {rc}"}
            dump()
            log(f"{name}: step ended with status {rc}; stopping")
            return 1
        with open(tmp) as f:
            out["indexes"][name] = json.load(f)
        os.remove(tmp)
        dump()
    log(json.dumps({n: r.get("alternating") for n, r in out["indexes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
