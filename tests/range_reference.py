"""CPU reference of range search on the exact-distance walk (CANON 19), composed from the oracle's exported stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``Reference.evaluated`` restates the loop of ``exact_reference.Reference.search_one`` in
mode ``exact`` and records, beside what that loop returns, the survivors of EVERY iteration in input order with the distances the walk computed --
the first iteration with its seed list, and the cap iteration, whose survivors are evaluated but never merged.  The walk reads no radius, so one
trace serves every radius, capacity and exclusion set.  ``collect`` then builds a query's answer from its trace:

    hit(x)   =  dist(x) <= radius (a float32 compare: NaN and negative radii admit nothing) and x not in excluded
    offered  =  the hits of all iterations, in evaluation order;  kept = the first cap of them
    answer   =  kept, sorted ascending by the key (distance bits << 32) | id, equal keys once;  count = its length
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

import exact_reference as XR
import labels_reference as LR

PAD_ID = LR.PAD_ID
BIG_DIST = XR.BIG_DIST
MARK0 = 0x01010101


class Trace:
    """One query's walk: iters = [(iteration, ids u32, dists f32)] for every iteration that evaluated a survivor (the last, unmerged one included),
    wl_ids / wl_dists the final worklist, stats (iterations, candidates, dist_evals, fetched), log the expanded nodes."""
    __slots__ = ("iters", "wl_ids", "wl_dists", "stats", "log")


class Reference(LR.Reference):
    def evaluated(self, query: np.ndarray, L: int) -> Trace:
        ix = self.ix
        q = np.ascontiguousarray(query, dtype=O.NP_DTYPE[ix.dtype])
        medoid = int(ix.medoid)
        max_cand = L + XR.EXTRA_ITERS
        bloom = np.zeros(O.BF_MEMORY, dtype=np.uint8)
        cand = [medoid]
        T = np.concatenate([np.array([medoid], np.uint32), self.adjacency(medoid)])
        it = 1
        fetched = len(T)
        S = O.filter_ids(bloom, T)                                       # K5
        d = self.exact(S, q)                                             # CANON 10
        evals = len(S)
        mark = MARK0
        has_parent, parent, mk = O.parent1(S, d, medoid)                 # K4a
        if has_parent:
            mark = mk
            cand.append(parent)
        wi = np.zeros(0, np.uint32)
        wd = np.zeros(0, np.float32)
        wv = np.zeros(0, np.uint8)
        iters = []
        while has_parent or len(S) > 0:
            if len(S):
                iters.append((it, S.copy(), d.copy()))                   # CANON 19: what the hit test sees, in input order
            S, d = O.sort_pairs(S, d)                                    # K3a
            wi, wd, wv = O.merge(S, d, it, wi, wd, wv, L, medoid, mark)  # K3b
            T = self.adjacency(parent) if has_parent else np.zeros(0, np.uint32)
            fetched += len(T)
            S = O.filter_ids(bloom, T)
            d = self.exact(S, q)
            evals += len(S)
            it += 1
            has_parent, parent, mark, wv = O.parent2(S, d, wi, wd, wv, medoid, mark)   # K4b
            if has_parent:
                cand.append(parent)
            if it == max_cand - 1:
                break
        if len(S):                                                       # the cap iteration: evaluated, not merged -- its hits count all the same
            iters.append((it, S.copy(), d.copy()))
        t = Trace()
        t.iters, t.wl_ids, t.wl_dists, t.stats, t.log = iters, wi, wd, (it, len(cand), evals, fetched), np.array(cand, np.uint32)
        return t

    def evaluated_all(self, queries: np.ndarray, L: int):
        return [self.evaluated(queries[i], L) for i in range(queries.shape[0])]


def hits(trace: Trace, radius, excluded=None):
    """-> (ids u32, dists f32, iteration of each) of ALL hits in evaluation order"""
    r = np.float32(radius)
    ids, dists, its = [], [], []
    for it, S, d in trace.iters:
        with np.errstate(invalid="ignore"):
            m = d <= r
        if excluded is not None and len(excluded):
            m &= ~np.isin(S, np.asarray(excluded, np.uint32))
        ids.append(S[m]); dists.append(d[m]); its.append(np.full(int(m.sum()), it, np.int64))
    if not ids:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    return np.concatenate(ids).astype(np.uint32), np.concatenate(dists).astype(np.float32), np.concatenate(its)


def keys(ids, dists) -> np.ndarray:
    return (np.ascontiguousarray(dists, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def collect(trace: Trace, radius, cap: int, excluded=None):
    """-> (ids u64 [count], dists f32 [count], offered, count): the query's answer"""
    ids, dists, _ = hits(trace, radius, excluded)
    offered = len(ids)
    k = np.unique(keys(ids[:cap], dists[:cap]))                          # sorted ascending, equal keys once
    out_ids = (k & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    out_d = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return out_ids, out_d, offered, len(k)


def collect_all(traces, radii, cap: int, excluded=None):
    """-> (lims u64 [Q + 1], ids u64, dists f32, counts u32 [Q], offered u32 [Q]): the batch's answer packed CSR in query order"""
    Q = len(traces)
    lims = np.zeros(Q + 1, np.uint64)
    counts = np.zeros(Q, np.uint32)
    offered = np.zeros(Q, np.uint32)
    ids, dists = [], []
    for i, t in enumerate(traces):
        a, b, offered[i], counts[i] = collect(t, radii[i], cap, excluded)
        ids.append(a); dists.append(b)
        lims[i + 1] = lims[i] + np.uint64(counts[i])
    return (lims, np.concatenate(ids) if ids else np.zeros(0, np.uint64), np.concatenate(dists) if dists else np.zeros(0, np.float32), counts,
            offered)
