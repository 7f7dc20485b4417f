"""CPU reference of per-query label filters on the exact-distance walk (CANON 18), composed from the oracle's exported stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``Reference.walk`` restates the loop of ``exact_reference.Reference.search_one`` in
mode ``exact`` and records, beside what that loop returns, the survivors of every iteration that is merged into the worklist -- in input order, with
the distances the walk computed.  The walk reads neither labels nor filters, so one trace serves every table and filter.  ``collect`` then builds
the RESULT LIST of a query from its trace: the matching survivors of each merged iteration go through ``O.sort_pairs`` / ``O.merge`` -- the
worklist's own K3a + K3b -- into a second list of capacity L.  ``orc_merge`` reads ``w_dist[w_n - 1]`` at ``iter > 1``, so an empty list is merged
into with ``iter = 1`` (which yields the first min(n, L) sorted survivors) and a non-empty one with ``iter = 2``.

    match(x)  =  (any == 0 or labels[x] & any != 0) and labels[x] & all == all and x not in excluded
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

import exact_reference as XR

PAD_ID = np.iinfo(np.uint64).max
BIG_DIST = XR.BIG_DIST
MARK0 = 0x01010101


class Trace:
    """One query's walk: merged = [(iteration, ids u32, dists f32)] for every iteration whose survivors were merged, wl_ids / wl_dists the final
    worklist, stats (iterations, candidates, dist_evals, fetched), log the expanded nodes."""
    __slots__ = ("merged", "wl_ids", "wl_dists", "stats", "log")


class Reference(XR.Reference):
    def walk(self, query: np.ndarray, L: int) -> Trace:
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
        merged = []
        while has_parent or len(S) > 0:
            merged.append((it, S.copy(), d.copy()))                      # CANON 18: what the result list is offered, in input order
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
        t = Trace()
        t.merged, t.wl_ids, t.wl_dists, t.stats, t.log = merged, wi, wd, (it, len(cand), evals, fetched), np.array(cand, np.uint32)
        return t

    def walks(self, queries: np.ndarray, L: int):
        return [self.walk(queries[i], L) for i in range(queries.shape[0])]


def matches(ids, labels, any_, all_, excluded=None) -> np.ndarray:
    lab = np.asarray(labels, np.uint32)[np.asarray(ids, np.int64)]
    any_, all_ = np.uint32(any_), np.uint32(all_)
    m = ((lab & any_) != 0) if int(any_) != 0 else np.ones(len(lab), bool)
    m &= (lab & all_) == all_
    if excluded is not None and len(excluded):
        m &= ~np.isin(np.asarray(ids, np.uint32), np.asarray(excluded, np.uint32))
    return m


def collect(trace: Trace, labels, any_: int, all_: int, k: int, L: int, medoid: int, excluded=None):
    """-> (ids u64 [k], dists f32 [k], matched, first, sizes): first = the iteration of the first non-empty merge into the result list (0: none),
    sizes = the matching survivors of every merged iteration"""
    ri = np.zeros(0, np.uint32)
    rd = np.zeros(0, np.float32)
    rv = np.zeros(0, np.uint8)
    matched, first, sizes = 0, 0, []
    for it, S, d in trace.merged:
        m = matches(S, labels, any_, all_, excluded)
        n = int(m.sum())
        sizes.append(n)
        if n == 0:
            continue
        matched += n
        if first == 0:
            first = it
        Ms, Md = O.sort_pairs(S[m], d[m])
        ri, rd, rv = O.merge(Ms, Md, 1 if len(ri) == 0 else 2, ri, rd, rv, L, medoid, MARK0)
    ids = np.full(k, PAD_ID, np.uint64)
    dists = np.full(k, BIG_DIST, np.float32)
    n = min(k, len(ri))
    ids[:n] = ri[:n]
    dists[:n] = rd[:n]
    return ids, dists, matched, first, sizes


def collect_all(traces, labels, any_, all_, k: int, L: int, medoid: int, excluded=None):
    """-> ids u64 [Q][k], dists f32 [k][Q] (rank-major), matched u32 [Q], stats int64 [Q][4], first [Q]"""
    Q = len(traces)
    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((k, Q), np.float32)
    matched = np.zeros(Q, np.uint32)
    first = np.zeros(Q, np.int64)
    st = np.empty((Q, 4), np.int64)
    for i, t in enumerate(traces):
        ids[i], dists[:, i], matched[i], first[i], _ = collect(t, labels, int(any_[i]), int(all_[i]), k, L, medoid, excluded)
        st[i] = t.stats
    return ids, dists, matched, st, first


def worklist_pick(trace: Trace, labels, any_: int, all_: int, k: int, excluded=None):
    """The post-filter composition, for comparison: the first k matching entries of the FINAL worklist."""
    m = matches(trace.wl_ids, labels, any_, all_, excluded) if len(trace.wl_ids) else np.zeros(0, bool)
    ids = np.full(k, PAD_ID, np.uint64)
    dists = np.full(k, BIG_DIST, np.float32)
    n = min(k, int(m.sum()))
    ids[:n] = trace.wl_ids[m][:n]
    dists[:n] = trace.wl_dists[m][:n]
    return ids, dists
