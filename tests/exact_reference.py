"""CPU reference of the exact-distance search mode (option ``distance`` = 1), composed from the oracle's exported stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``search_one`` restates the oracle's whole-query loop (oracle/bang_oracle.c
search_one: seeding, K5 filter, distance stage, K4 parent, K3a sort + K3b merge, the L + 49 cap) with two stages switchable:

* ``pq``    -- K1 ``orc_lut_build`` + K2 ``orc_pqdist`` in the walk, then the re-rank of the candidate log (K6 ``orc_exact_dist`` + K7 ``orc_topk``):
               the BANG_Base search, equal to ``Oracle.search`` bit for bit (tests/test_exact_mode.py pins the composition to it);
* ``exact`` -- every survivor's distance is ``orc_exact_dist`` of the node's vector (the first D elements of its graph entry) against the RAW
               query, and the results are the first min(k, w_n) worklist entries as the loop leaves them -- at the iteration cap the last
               iteration's survivors are not merged -- padded with UINT64_MAX / 3.402823E+38 (CANON 10 and 11).

Adjacency is read from the index's graph entries ([vec][u32 degree][u32 id x R]).  Per-query statistics are (iterations, candidates,
dist_evals, fetched), the oracle's column order; ``candidates`` = nodes expanded, the medoid included.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O

BIG_DIST = np.float32(3.402823e38)
EXTRA_ITERS = 50
MODES = ("pq", "exact")


class Reference:
    def __init__(self, ix):
        self.ix = ix
        self.orc = O.Oracle(ix)
        self.tsize = 4 if ix.dtype == "float" else 1
        self.graph = self.orc.graph                                      # uint8 [N][entry_len]
        self._gbase = self.graph.ctypes.data
        self._entry_len = int(ix.entry_len)
        self._dcode = C.c_int(O.DTYPE_CODE[ix.dtype])

    def adjacency(self, node: int) -> np.ndarray:
        off = self.ix.D * self.tsize
        e = self.graph[node]
        deg = min(int(e[off:off + 4].view(np.uint32)[0]), self.ix.R)
        return e[off + 4: off + 4 + 4 * deg].view(np.uint32).copy()

    def exact(self, ids: np.ndarray, query: np.ndarray) -> np.ndarray:
        """orc_exact_dist of every id's vector against the raw query (no MIPS padding)."""
        fn = O.lib().orc_exact_dist
        qp = C.c_void_p(query.ctypes.data)
        D = C.c_uint32(self.ix.D)
        out = np.empty(len(ids), dtype=np.float32)
        for i, x in enumerate(ids):
            out[i] = fn(C.c_void_p(self._gbase + int(x) * self._entry_len), qp, D, self._dcode, C.c_int(0))
        return out

    def search_one(self, query: np.ndarray, k: int, L: int, mode: str):
        """-> (ids u64 [k], dists f32 [k], stats (iterations, candidates, dist_evals, fetched))"""
        if mode not in MODES:
            raise ValueError(mode)
        ix = self.ix
        q = np.ascontiguousarray(query, dtype=O.NP_DTYPE[ix.dtype])
        medoid = int(ix.medoid)
        max_cand = L + EXTRA_ITERS
        bloom = np.zeros(O.BF_MEMORY, dtype=np.uint8)
        if mode == "pq":
            lut = self.orc.lut_build(q)
            dist = lambda s: self.orc.pqdist(lut, s)                     # noqa: E731  K2
        else:
            dist = lambda s: self.exact(s, q)                            # noqa: E731  CANON 10
        cand = [medoid]
        T = np.concatenate([np.array([medoid], np.uint32), self.adjacency(medoid)])
        it = 1
        fetched = len(T)
        S = O.filter_ids(bloom, T)                                       # K5
        d = dist(S)
        evals = len(S)
        mark = 0x01010101
        has_parent, parent, mk = O.parent1(S, d, medoid)                 # K4a
        if has_parent:
            mark = mk
            cand.append(parent)
        wi = np.zeros(0, np.uint32)
        wd = np.zeros(0, np.float32)
        wv = np.zeros(0, np.uint8)
        while has_parent or len(S) > 0:
            S, d = O.sort_pairs(S, d)                                    # K3a
            wi, wd, wv = O.merge(S, d, it, wi, wd, wv, L, medoid, mark)  # K3b
            T = self.adjacency(parent) if has_parent else np.zeros(0, np.uint32)
            fetched += len(T)
            S = O.filter_ids(bloom, T)
            d = dist(S)
            evals += len(S)
            it += 1
            has_parent, parent, mark, wv = O.parent2(S, d, wi, wd, wv, medoid, mark)   # K4b
            if has_parent:
                cand.append(parent)
            if it == max_cand - 1:
                break
        if mode == "pq":                                                 # K6 + K7
            cd = self.exact(np.array(cand, np.uint32), q)
            ids, dists = O.topk(np.array(cand, np.uint32), cd, k)
        else:                                                            # CANON 11: the worklist as it stands
            ids = np.full(k, np.iinfo(np.uint64).max, dtype=np.uint64)
            dists = np.full(k, BIG_DIST, dtype=np.float32)
            n = min(k, len(wi))
            ids[:n] = wi[:n]
            dists[:n] = wd[:n]
        return ids, dists, (it, len(cand), evals, fetched)

    def search(self, queries: np.ndarray, k: int, L: int, mode: str):
        """-> ids u64 [Q][k], dists f32 [k][Q] (rank-major), stats int64 [Q][4] (iterations, candidates, dist_evals, fetched)"""
        Q = queries.shape[0]
        ids = np.empty((Q, k), np.uint64)
        dists = np.empty((k, Q), np.float32)
        st = np.empty((Q, 4), np.int64)
        for i in range(Q):
            ids[i], dists[:, i], st[i] = self.search_one(queries[i], k, L, mode)
        return ids, dists, st
