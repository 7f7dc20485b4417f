"""CPU reference of the BANG_Inmemory search semantics (option ``semantics`` = 1), composed from the oracle's exported stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``search_one`` restates the whole-query loop with the walk switchable:

* ``base``     -- the oracle's loop (oracle/bang_oracle.c search_one): K4 picks the parent BEFORE the merge (compute_parent1 / compute_parent2,
                  strict '<' against the first unvisited entry, the corner case against the tail), merges with the reference's mark, and stops at
                  iteration L + 49.  Equal to ``Oracle.search`` bit for bit (tests/test_inmemory_mode.py pins the composition to it).
* ``inmemory`` -- BANG_Inmemory/parANN.cu:964-1016, :1287-1420: the survivors are sorted and merged with a
                  mark no id equals, THEN the parent is the first unvisited worklist entry, marked visited; a query without one ends.  The loop
                  stops at iteration L + 119 (candidate log of L + 120): the parent picked there is logged and re-ranked but never expanded.

Both re-rank the candidate log (K6 ``orc_exact_dist`` + K7 ``orc_topk``).  Adjacency is read from the index's graph entries
([vec][u32 degree][u32 id x R]).  Per-query statistics are (iterations, candidates, dist_evals, fetched), the oracle's column order.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

EXTRA_ITERS = {"base": 50, "inmemory": 120}
NO_MARK = 0xFFFFFFFF
MODES = ("base", "inmemory")


class Reference:
    def __init__(self, ix):
        self.ix = ix
        self.orc = O.Oracle(ix)
        self.tsize = 4 if ix.dtype == "float" else 1
        self.graph = self.orc.graph                                      # uint8 [N][entry_len]

    def adjacency(self, node: int) -> np.ndarray:
        off = self.ix.D * self.tsize
        e = self.graph[node]
        deg = min(int(e[off:off + 4].view(np.uint32)[0]), self.ix.R)
        return e[off + 4: off + 4 + 4 * deg].view(np.uint32).copy()

    def search_one(self, query: np.ndarray, k: int, L: int, mode: str):
        """-> (ids u64 [k], dists f32 [k], stats (iterations, candidates, dist_evals, fetched))"""
        return self.search_one_logged(query, k, L, mode)[:3]

    def search_one_logged(self, query: np.ndarray, k: int, L: int, mode: str):
        """search_one, and the candidate log behind it: -> (ids, dists, stats, candidates u32 [stats[1]], the expanded nodes in order)"""
        if mode not in MODES:
            raise ValueError(mode)
        ix = self.ix
        q = np.ascontiguousarray(query, dtype=O.NP_DTYPE[ix.dtype])
        medoid = int(ix.medoid)
        cap = L + EXTRA_ITERS[mode] - 1
        bloom = np.zeros(O.BF_MEMORY, dtype=np.uint8)
        lut = self.orc.lut_build(q)
        cand = [medoid]
        wi = np.zeros(0, np.uint32)
        wd = np.zeros(0, np.float32)
        wv = np.zeros(0, np.uint8)
        T = np.concatenate([np.array([medoid], np.uint32), self.adjacency(medoid)])
        it = 1
        fetched = len(T)
        evals = 0
        if mode == "inmemory":
            while True:
                S = O.filter_ids(bloom, T)                               # K5
                d = self.orc.pqdist(lut, S)                              # K2
                evals += len(S)
                S, d = O.sort_pairs(S, d)                                # K3a
                wi, wd, wv = O.merge(S, d, it, wi, wd, wv, L, medoid, NO_MARK)   # K3b, no d_mark step
                unvisited = np.flatnonzero(wv == 0)                      # the parent AFTER the merge (:1399-1418)
                if len(unvisited) == 0:
                    break
                i = int(unvisited[0])
                wv[i] = 1
                cand.append(int(wi[i]))
                if it == cap:                                            # _DBG break, MAX_PARENTS_PERQUERY = L + 120 (:30, :603-609)
                    break
                T = self.adjacency(int(wi[i]))
                fetched += len(T)
                it += 1
        else:                                                            # the oracle's loop (tests/exact_reference.py, pq mode)
            S = O.filter_ids(bloom, T)
            d = self.orc.pqdist(lut, S)
            evals = len(S)
            mark = 0x01010101
            has_parent, parent, mk = O.parent1(S, d, medoid)             # K4a
            if has_parent:
                mark = mk
                cand.append(parent)
            while has_parent or len(S) > 0:
                S, d = O.sort_pairs(S, d)
                wi, wd, wv = O.merge(S, d, it, wi, wd, wv, L, medoid, mark)
                T = self.adjacency(parent) if has_parent else np.zeros(0, np.uint32)
                fetched += len(T)
                S = O.filter_ids(bloom, T)
                d = self.orc.pqdist(lut, S)
                evals += len(S)
                it += 1
                has_parent, parent, mark, wv = O.parent2(S, d, wi, wd, wv, medoid, mark)   # K4b
                if has_parent:
                    cand.append(parent)
                if it == cap:
                    break
        c = np.array(cand, np.uint32)                                    # K6 + K7
        cd = np.array([self.orc.exact_dist(int(x), q) for x in c], np.float32)
        ids, dists = O.topk(c, cd, k)
        return ids, dists, (it, len(cand), evals, fetched), c

    def search(self, queries: np.ndarray, k: int, L: int, mode: str):
        """-> ids u64 [Q][k], dists f32 [k][Q] (rank-major), stats int64 [Q][4] (iterations, candidates, dist_evals, fetched)"""
        Q = queries.shape[0]
        ids = np.empty((Q, k), np.uint64)
        dists = np.empty((k, Q), np.float32)
        st = np.empty((Q, 4), np.int64)
        for i in range(Q):
            ids[i], dists[:, i], st[i] = self.search_one(queries[i], k, L, mode)
        return ids, dists, st


def toy_index(adj: dict, levels: list, medoid: int = 0, R: int = 64):
    """A hand-made uint8 index (D = 128, m = 32: chunks of 4 dimensions, a layout the search kernel has an instance for) in which the
    walk is known in advance.  Node i's vector is levels[i] in every dimension and so is every one of its PQ codes; pivot c is c in every
    dimension and the centroid is 0.  For the all-zero query the PQ distance of node i is then 128 levels[i]^2 and so is its exact distance
    -- integers below 2^24, exact in float in any order: equal levels are exact ties, a falling level is a falling distance."""
    from bang_amd.formats import Index, pack_graph
    N, D, m = len(levels), 128, 32
    lv = np.asarray(levels, np.uint8)
    vec = np.repeat(lv[:, None], D, axis=1)
    deg = np.zeros(N, np.uint32)
    nbr = np.zeros((N, R), np.uint32)
    for i, row in adj.items():
        deg[i] = len(row)
        nbr[i, :len(row)] = row
    graph = pack_graph(vec, deg, nbr)
    pivots = np.repeat(np.arange(256, dtype=np.float32)[:, None], D, axis=1)
    ix = Index(dtype="uint8", N=N, D=D, R=R, m=m, medoid=medoid, graph=graph, codes=np.repeat(lv[:, None], m, axis=1).copy(),
               pivots=pivots, centroid=np.zeros(D, np.float32), chunk_off=np.arange(0, D + 1, D // m, dtype=np.uint32))
    return ix, np.zeros((1, D), np.uint8)


def chain_index(n: int = 256):
    """0 -> 1 -> ... -> n - 1, level 255 - i: the PQ distance falls strictly along the chain, so the walk runs to the iteration cap."""
    return toy_index({i: [i + 1] for i in range(n - 1)}, [255 - i for i in range(n)])


def tie_index():
    """The best survivor ties with the first unvisited worklist entry (node 3 vs node 2, both at level 20): BANG_Base keeps the old entry,
    the merge puts the new one first.  At L = 3 the two walks then evict different nodes and log different candidates."""
    return toy_index({0: [1, 2], 1: [3], 2: [4], 3: [5]}, [200, 10, 20, 20, 5, 6])


def not_full_index():
    """A worklist that is not full and has no unvisited entry takes a survivor no better than its tail (node 2 behind the medoid):
    BANG_Base expands it one iteration later than the merge-first rule."""
    return toy_index({0: [1], 1: [2], 2: [3]}, [50, 10, 100, 1])


def medoid_tie_index():
    """The medoid ties its best neighbour (node 1, both at level 10): on iteration 1 the stable sort keeps the medoid in front of the
    parent, so the parent is NOT at the slot a count of closer entries names.  Expanded once, node 1 leaves the walk 0, 1, 3, 2, 4."""
    return toy_index({0: [1, 2], 1: [3], 2: [4]}, [10, 10, 20, 5, 6])


def medoid_tie_variant(ix, q):
    """A fixture with the medoid's code row replaced by that of its first neighbour j, and every query moved onto j's vector: on iteration 1
    the medoid and j tie, and j is the best survivor."""
    import dataclasses
    adj, deg = ix.adjacency(), ix.degrees()
    j = int(adj[ix.medoid][0])
    assert deg[ix.medoid] > 0
    codes = ix.codes.copy()
    codes[ix.medoid] = ix.codes[j]
    qq = np.repeat(ix.vectors()[j][None, :], q.shape[0], axis=0).astype(q.dtype)
    return dataclasses.replace(ix, codes=codes), np.ascontiguousarray(qq), j
