"""CPU reference of the beam form of the exact-distance search (options ``distance`` = 1, ``beam`` = W), composed from the oracle's stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``search_one`` restates DESIGN.md section 4.10 (CANON 14 and 15):

    cand = [medoid]; rows = [[medoid] + adj(medoid)]; it = 1; worklist empty; filter empty
    loop:
      1. T = rows[0] | rows[1] | ...: every id is tested against the filter state AT ENTRY of the iteration, then the bits of every id that
         passed are set (``O.filter_ids`` on the concatenation: CANON 3 over all rows at once).          fetched += len(T)
      2. a survivor of rows[j] whose id also survived in a row i < j is dropped; duplicates inside one row stay.  S_j = what is left.
      3. ``orc_exact_dist`` of every kept survivor against the raw query.                                dist_evals += sum len(S_j)
      4. for j = 0, 1, ...: K3a ``O.sort_pairs`` (stable), K3b ``O.merge`` with mark = NO_MARK; the merge's iteration argument is 1 for the
         seed list and 2 for every later row (among equal distances a later row's entry stands in front of an earlier row's).
      5. P = min(W, cand_stride - len(cand), unvisited worklist entries): the first P unvisited entries are marked and appended to cand.
         P == 0: the query ends.
      6. it == cap (L + 49): the query ends; these parents are logged, never expanded.
      7. rows = [adj(p) for the P parents, in that order]; it += 1
    results: the first min(k, w_n) worklist entries, padded with UINT64_MAX / 3.402823e38 (CANON 11).

Which ids of T survive is one bit per id -- every copy of an id has the same outcome against the state at entry -- so the survivors' positions
are ``np.isin(T, S)``.  Per-query statistics are (iterations, candidates, dist_evals, fetched), the oracle's column order.  ``trace``, where
given, receives one dict per iteration: what the edge-input assertions of tests/test_beam_mode.py look at.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from exact_reference import Reference as ExactReference
from inmemory_reference import NO_MARK

BIG_DIST = np.float32(3.402823e38)
EXTRA_ITERS = 50


class Reference(ExactReference):
    def search_one(self, query: np.ndarray, k: int, L: int, W: int, trace: list | None = None):
        """-> (ids u64 [k], dists f32 [k], stats (iterations, candidates, dist_evals, fetched), candidates u32 [stats[1]])"""
        if not 1 <= W <= 4:
            raise ValueError(W)
        ix = self.ix
        q = np.ascontiguousarray(query, dtype=O.NP_DTYPE[ix.dtype])
        medoid = int(ix.medoid)
        cand_stride, cap = L + EXTRA_ITERS, L + EXTRA_ITERS - 1
        bloom = np.zeros(O.BF_MEMORY, dtype=np.uint8)
        cand = [medoid]
        rows = [np.concatenate([np.array([medoid], np.uint32), self.adjacency(medoid)])]
        wi, wd, wv = np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint8)
        it, fetched, evals = 1, 0, 0
        while True:
            T = np.concatenate(rows)                                     # step 1
            fetched += len(T)
            S = O.filter_ids(bloom, T)
            passed = np.isin(T, S)
            kept, seen, dropped, o = [], set(), 0, 0                     # step 2
            for r in rows:
                ids = r[passed[o:o + len(r)]]
                o += len(r)
                keep = np.array([int(x) not in seen for x in ids], bool)
                dropped += int((~keep).sum())
                kept.append(ids[keep])
                seen.update(int(x) for x in ids)
            for j, s_ids in enumerate(kept):                             # steps 3 and 4
                d = self.exact(s_ids, q)
                evals += len(s_ids)
                s_ids, d = O.sort_pairs(s_ids, d)
                wi, wd, wv = O.merge(s_ids, d, 1 if it == 1 else 2, wi, wd, wv, L, medoid, NO_MARK)
            unvisited = np.flatnonzero(wv == 0)                          # step 5
            P = min(W, cand_stride - len(cand), len(unvisited))
            parents = [int(wi[i]) for i in unvisited[:P]]
            wv[unvisited[:P]] = 1
            cand += parents
            if trace is not None:
                trace.append(dict(it=it, rows=len(rows), kept=[len(s) for s in kept], dropped=dropped, unvisited=len(unvisited), P=P,
                                  room=cand_stride - (len(cand) - P), parents=parents))
            if P == 0 or it == cap:                                      # step 6
                break
            rows = [self.adjacency(p) for p in parents]                  # step 7
            it += 1
        ids = np.full(k, np.iinfo(np.uint64).max, dtype=np.uint64)
        dists = np.full(k, BIG_DIST, dtype=np.float32)
        n = min(k, len(wi))
        ids[:n] = wi[:n]
        dists[:n] = wd[:n]
        return ids, dists, (it, len(cand), evals, fetched), np.array(cand, np.uint32)

    def search(self, queries: np.ndarray, k: int, L: int, W: int):
        """-> ids u64 [Q][k], dists f32 [k][Q] (rank-major), stats int64 [Q][4], candidate log u32 [Q][L + 50] (zero behind a query's count)"""
        Q = queries.shape[0]
        ids = np.empty((Q, k), np.uint64)
        dists = np.empty((k, Q), np.float32)
        st = np.empty((Q, 4), np.int64)
        log = np.zeros((Q, L + EXTRA_ITERS), np.uint32)
        for i in range(Q):
            ids[i], dists[:, i], st[i], c = self.search_one(queries[i], k, L, W)
            log[i, :len(c)] = c
        return ids, dists, st, log
