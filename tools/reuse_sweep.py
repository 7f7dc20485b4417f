#!/usr/bin/env python3
"""An index under churn (Engine.insert_reuse): does N stay put, what does recall do over generations, and what does the id
indirection cost against the appending insert.  Graph in HBM, capacity == N.

Workloads: the structured synthetic 10^6-point indexes of tools/consolidate_sweep.py / tools/insert_sweep.py (sift1m: uint8, D = 128, m = 32;
deep1m: float, D = 96, m = 74; R = 64), built by synth.build_graph / synth.train_pq.

  churn    --generations times: exclude a random 10 % of the nodes (never the medoid), Engine.consolidate, then Engine.insert_reuse the same number
           of fresh points of the same distribution in batches of --batch.  Per generation: N (which must not grow), Engine.free_slots(), the
           consolidation's wall time, points/s of the inserts (host wall time over all batches), and 10-recall@10 of the exact and the PQ walk
           over --Ls against Engine.scan of the same engine as truth.  --rebuild names the generations after which an index is also BUILT over
           that generation's live vectors and measured the same way (against its own scan): what the churned graph loses to a fresh one.
  cost     f = n: --runs batches of --batch points through Engine.insert_reuse on an engine with that many free slots, against Engine.insert on a
           twin engine loaded from the same consolidated export, alternating in one process; medians, the ratio, and the phases of
           bang_get_insert_times for both.

There is no threshold: the numbers are a record.

  python tools/reuse_sweep.py --workloads sift1m,deep1m --out profiles/reuse.json --md profiles/reuse_tables.md

Not part of bench.py: the measurement behind profiles/reuse.md.
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
import insert_sweep  # noqa: E402

PHASES = ("search", "prune", "group", "backedge", "encode", "total")


def recall_rows(e, q, Ls, k, tag, log):
    """10-recall@10 of the exact and the PQ walk against the engine's own exact scan"""
    gi, gd, _ = e.scan(q, k)
    gd = np.ascontiguousarray(gd.T)
    rows = []
    for walk, distance in (("exact", 1), ("pq", 0)):
        e.set_option("distance", distance)
        e.set_option("search", 1)
        for L in Ls:
            e.set_searchparams(k, L)
            e.alloc(q.shape[0])
            e.init(q.shape[0])
            ids, _ = e.query(q)
            e.free()
            row = dict(tag, walk=walk, L=L, recall=round(O.recall(gi.astype(np.uint32), gd, ids, k), 3))
            log(json.dumps(row))
            rows.append(row)
    return rows


def markdown(out):
    s = []
    for w in out["workloads"]:
        name = w["name"]
        s += [f"### {name}: N = {w['N']}, D = {w['D']}, {w['dtype']}, R = {w['R']}, m = {w['m']}; capacity = N; alpha = {out['alpha']}, L_build = {out['L_build']}, "
              f"batches of {out['batch']}", "",
              "| generation | deleted | consolidate s | inserted | points/s | N | free / eligible behind the inserts | slots reused since the load |", "|---|---|---|---|---|---|---|---|"]
        for g in (g for g in out["churn"] if g["workload"] == name):
            s.append(f"| {g['generation']} | {g['deleted']} | {g['consolidate_s']:.1f} | {g['inserted']} | {g['pps']:.0f} | {g['N']} | {g['free']} / {g['eligible']} | {g['reused']} |")
        rec = {(r["index"], r["generation"], r["walk"], r["L"]): r["recall"] for r in out["recall"] if r["workload"] == name}
        gens = sorted({r["generation"] for r in out["recall"] if r["workload"] == name})
        s += ["", "10-recall@10 against `Engine.scan` of the same engine; churned / rebuilt over that generation's live vectors (- : not rebuilt)", "",
              "| walk | L | " + " | ".join(f"gen {g}" for g in gens) + " |", "|---|---|" + "---|" * len(gens)]
        for walk in ("exact", "pq"):
            for L in out["Ls"]:
                cells = []
                for g in gens:
                    a, b = rec.get(("churned", g, walk, L)), rec.get(("rebuilt", g, walk, L))
                    cells.append((f"{a:.2f}" if a is not None else "-") + " / " + (f"{b:.2f}" if b is not None else "-"))
                s.append(f"| {walk} | {L} | " + " | ".join(cells) + " |")
        c = next((c for c in out["cost"] if c["workload"] == name), None)
        if c:
            s += ["", f"f = n = {out['batch']}, medians of {c['runs']} alternating runs, ms per call (bang_get_insert_times; `group` holds the select of E, the entries to their "
                  "slots and the rows down, `encode` the code rows to their slots)", "", "| call | " + " | ".join(PHASES) + " | wall |", "|---|" + "---|" * (len(PHASES) + 1)]
            for call in ("insert_reuse", "insert"):
                s.append(f"| {call} | " + " | ".join(f"{c[call][p]:.2f}" for p in PHASES) + f" | {c[call]['wall']:.2f} |")
            s += ["", f"insert_reuse / insert (wall, medians): {c['ratio']:.3f}"]
        s.append("")
    return "\n".join(s) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="sift1m,deep1m")
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--rebuild", default="all", help="generations after which an index is built over the live vectors: all, none, or a list (1,5)")
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--Ls", default="22,46,94,190")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--L_build", type=int, default=64)
    ap.add_argument("--alpha", type=float, default=1.2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="", help="raw JSON")
    ap.add_argument("--md", default="", help="the tables as markdown")
    a = ap.parse_args()
    log = lambda s: print(s, flush=True)                     # noqa: E731
    if bang_amd.device_count() < 1:
        raise SystemExit("reuse_sweep needs a HIP device: nothing here is measured on a CPU")
    import torch
    k = 10
    Ls = [int(x) for x in a.Ls.split(",")]
    rebuild = set(range(1, a.generations + 1)) if a.rebuild == "all" else set() if a.rebuild == "none" else {int(x) for x in a.rebuild.split(",")}
    out = {"k": k, "alpha": a.alpha, "L_build": a.L_build, "batch": a.batch, "Ls": Ls, "workloads": [], "churn": [], "recall": [], "cost": []}

    def flush():
        for path, text in ((a.out, json.dumps(out, indent=1)), (a.md, markdown(out))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(text)

    for name in a.workloads.split(","):
        N, D, dtype, R, m, ncl = insert_sweep.WORKLOADS[name]
        seed = synth.SEED
        tenth = N // 10
        n_cost = a.runs * a.batch
        x = synth.make_vectors(N + a.generations * tenth + n_cost, D, dtype, n_clusters=ncl, seed=seed, device="cuda")
        x = x[torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed)).to(x.device)]     # (the fresh points are a random share)
        q = np.ascontiguousarray(synth.to_numpy(synth.make_queries(x[:N], a.queries, dtype, seed=seed), dtype))
        ix = insert_sweep.build(x[:N], dtype, R, m, seed, log, f"{name} generation 0")
        vec = np.ascontiguousarray(synth.to_numpy(x[:N], dtype))                                           # the live vectors by id
        fresh = np.ascontiguousarray(synth.to_numpy(x[N:], dtype))
        del x
        torch.cuda.empty_cache()
        out["workloads"].append({"name": name, "N": N, "D": D, "dtype": dtype, "R": R, "m": m})
        rng = np.random.default_rng(seed)
        e = bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE, capacity=N)
        e.load_index(ix)
        out["recall"] += recall_rows(e, q, Ls, k, dict(workload=name, index="churned", generation=0), log)
        at = 0
        for g in range(1, a.generations + 1):
            ids = rng.choice(N, tenth + 1, replace=False)
            ids = ids[ids != ix.medoid][:tenth].astype(np.uint32)
            e.set_excluded(ids)
            t0 = time.perf_counter()
            st = e.consolidate(a.alpha)
            t_cons = time.perf_counter() - t0
            t_ins = 0.0
            for b0 in range(0, tenth, a.batch):
                v = fresh[at + b0: at + min(b0 + a.batch, tenth)]
                t0 = time.perf_counter()
                got = e.insert_reuse(v, a.L_build, a.alpha)
                t_ins += time.perf_counter() - t0
                vec[got.astype(np.int64)] = v
            at += tenth
            fs = e.free_slots()
            row = dict(workload=name, generation=g, deleted=int(st["removed"]), consolidate_s=t_cons, inserted=tenth, pps=tenth / t_ins, N=e.num_nodes(),
                       free=fs["free"], eligible=fs["eligible"], reused=fs["reused"])
            log(json.dumps(row))
            assert row["N"] == N, "N grew although every batch fitted the free slots"
            out["churn"].append(row)
            out["recall"] += recall_rows(e, q, Ls, k, dict(workload=name, index="churned", generation=g), log)
            if g in rebuild:
                xr = torch.from_numpy(vec.astype(np.float32)).to("cuda")
                ixr = insert_sweep.build(xr, dtype, R, m, seed, log, f"{name} rebuilt at generation {g}")
                del xr
                torch.cuda.empty_cache()
                with bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE) as r:
                    r.load_index(ixr)
                    out["recall"] += recall_rows(r, q, Ls, k, dict(workload=name, index="rebuilt", generation=g), log)
                del ixr
            flush()                                           # (what is measured so far survives a time limit)
        # the cost of the indirection: f = n against the appending insert, twins of one consolidated export
        ids = rng.choice(N, n_cost + 1, replace=False)
        ids = ids[ids != ix.medoid][:n_cost].astype(np.uint32)
        e.set_excluded(ids)
        e.consolidate(a.alpha)
        exported, removed = e.export_index(ix), e.removed_ids()
        e.close()
        del ix
        twins = {}
        for call, cap in (("insert_reuse", N), ("insert", N + n_cost)):
            twins[call] = bang_amd.Engine(dtype, graph=bang_amd.GRAPH_DEVICE, capacity=cap)
            twins[call].load_index(exported)
        twins["insert_reuse"].set_removed(removed)
        times = {call: [] for call in twins}
        for r in range(a.runs):
            v = fresh[at + r * a.batch: at + (r + 1) * a.batch]
            for call in (("insert_reuse", "insert") if r % 2 == 0 else ("insert", "insert_reuse")):
                t0 = time.perf_counter()
                getattr(twins[call], call)(v, a.L_build, a.alpha)
                wall = 1e3 * (time.perf_counter() - t0)
                times[call].append(dict(twins[call].insert_times(), wall=wall))
        c = dict(workload=name, runs=a.runs)
        for call in twins:
            c[call] = {p: float(np.median([t[p] for t in times[call]])) for p in PHASES + ("wall",)}
            twins[call].close()
        c["ratio"] = c["insert_reuse"]["wall"] / c["insert"]["wall"]
        log(json.dumps(c))
        out["cost"].append(c)
        flush()
        del exported, vec, fresh
    flush()


if __name__ == "__main__":
    main()
