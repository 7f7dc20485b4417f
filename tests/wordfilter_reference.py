"""CPU reference of the word-local visited filter (option ``filter_layout`` = 1), composed from the oracle's exported stages.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``search_one`` is the whole-query loop of tests/exact_reference.py in its ``pq``
composition (seeding, K5 filter, K1 + K2 PQ distances, K4 parent, K3a sort + K3b merge, the L + 49 cap, K6 + K7 re-rank of the candidate log)
with the FILTER stage switchable:

* ``split`` -- ``oracle.filter_ids``: an id's two bits at hash1(x) and hash2(x), anywhere in the filter.  Equal to ``Oracle.search`` bit for bit
               (tests/test_wordfilter_mode.py pins the composition to it).
* ``word``  -- DESIGN.md section 2 row 16, restated here on ``oracle.hash1`` / ``oracle.hash2``: both bits in the 32-bit word of hash1(x),
               a = hash1(x), b = (hash1(x) & ~31) | ((hash2(x) >> 5) & 31); one bit where a == b.  Every id of a row is tested against the
               filter as it stood when the row arrived; an id is dropped iff all bits of its mask are set; the survivors, in input order,
               then set their masks (two survivors of one row that share a word are both kept).

MIPS: ``mips=True`` is the oracle's padding (``lut_build(q, 1)``, ``orc_exact_dist(..., 1)``).  Per-query statistics are (iterations,
candidates, dist_evals, fetched), the oracle's column order.  ``trace`` (a list) receives (iteration, ids offered, survivors) per filter call
and ``log`` the candidate log: the tests on the crafted inputs of tests/wordfilter_inputs.py read them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O

EXTRA_ITERS = 50
LAYOUTS = ("split", "word")
BF_WORDS = 12512                     # BANG_BF_WORDS: 32-bit words of one query's filter

_HASH = {}


def positions(x: int):
    """(hash1(x), hash2(x)) of the oracle, cached."""
    h = _HASH.get(x)
    if h is None:
        h = _HASH[x] = (O.hash1(int(x)), O.hash2(int(x)))
    return h


def word_of(x: int) -> int:
    return positions(x)[0] >> 5


def mask_of(x: int) -> int:
    a, b = positions(x)
    return (1 << (a & 31)) | (1 << ((b >> 5) & 31))


def filter_word(words: np.ndarray, ids) -> np.ndarray:
    """The word-local K5 on a filter of BF_WORDS uint32 words: tests all ids first (the snapshot), then sets the survivors' masks."""
    out = [int(x) for x in ids if (int(words[word_of(int(x))]) & mask_of(int(x))) != mask_of(int(x))]
    for x in out:
        words[word_of(x)] |= np.uint32(mask_of(x))
    return np.array(out, dtype=np.uint32)


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

    def exact(self, ids: np.ndarray, query: np.ndarray, dim_adjust: int) -> np.ndarray:
        fn = O.lib().orc_exact_dist
        qp = C.c_void_p(query.ctypes.data)
        D = C.c_uint32(self.ix.D)
        out = np.empty(len(ids), dtype=np.float32)
        for i, x in enumerate(ids):
            out[i] = fn(C.c_void_p(self._gbase + int(x) * self._entry_len), qp, D, self._dcode, C.c_int(dim_adjust))
        return out

    def search_one(self, query: np.ndarray, k: int, L: int, layout: str, mips: bool = False, trace=None, log=None):
        """-> (ids u64 [k], dists f32 [k], stats (iterations, candidates, dist_evals, fetched))"""
        if layout not in LAYOUTS:
            raise ValueError(layout)
        ix = self.ix
        q = np.ascontiguousarray(query, dtype=O.NP_DTYPE[ix.dtype])
        adjust = 1 if mips else 0
        medoid = int(ix.medoid)
        max_cand = L + EXTRA_ITERS
        if layout == "split":
            bloom = np.zeros(O.BF_MEMORY, dtype=np.uint8)
            flt = lambda t: O.filter_ids(bloom, t)                       # noqa: E731  K5, CANON 3
        else:
            words = np.zeros(BF_WORDS, dtype=np.uint32)
            flt = lambda t: filter_word(words, t)                        # noqa: E731  K5, CANON 16
        lut = self.orc.lut_build(q, adjust)                              # K1
        it = 1

        def k5(t):
            s = flt(t)
            if trace is not None:
                trace.append((it, np.array(t, np.uint32), s.copy()))
            return s

        cand = [medoid]
        T = np.concatenate([np.array([medoid], np.uint32), self.adjacency(medoid)])
        fetched = len(T)
        S = k5(T)
        d = self.orc.pqdist(lut, S)                                      # K2
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
            it += 1
            S = k5(T)
            d = self.orc.pqdist(lut, S)
            evals += len(S)
            has_parent, parent, mark, wv = O.parent2(S, d, wi, wd, wv, medoid, mark)   # K4b
            if has_parent:
                cand.append(parent)
            if it == max_cand - 1:
                break
        cd = self.exact(np.array(cand, np.uint32), q, adjust)            # K6
        ids, dists = O.topk(np.array(cand, np.uint32), cd, k)            # K7
        if log is not None:
            log.extend(cand)
        return ids, dists, (it, len(cand), evals, fetched)

    def search(self, queries: np.ndarray, k: int, L: int, layout: str, mips: bool = False):
        """-> ids u64 [Q][k], dists f32 [k][Q] (rank-major), stats int64 [Q][4] (iterations, candidates, dist_evals, fetched)"""
        Q = queries.shape[0]
        ids = np.empty((Q, k), np.uint64)
        dists = np.empty((k, Q), np.float32)
        st = np.empty((Q, 4), np.int64)
        for i in range(Q):
            ids[i], dists[:, i], st[i] = self.search_one(queries[i], k, L, layout, mips)
        return ids, dists, st
