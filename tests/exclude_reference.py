"""CPU reference of the excluded ids (lazy deletes, DESIGN.md section 2 CANON 17), composed from what the existing references return.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  The walk ignores the set X, so every walk-side quantity -- candidate log, worklist,
counters -- is that of the unmasked reference run; what changes is the composition behind it:

    masked_rerank     PQ walks: exact distances (orc_exact_dist) of the log entries NOT in X, in log order, then the stable top-k (O.topk), then
                      the padded tail
    masked_worklist   distance = 1: the first k entries of the final worklist (a reference run at k = L) that are not in X, in worklist order,
                      distance bits unchanged, then the padded tail

and the runners below return, per walk form, (ids u64 [Q][k], dists f32 [k][Q], stats int64 [Q][4], log u32 [Q][stride], counts [Q]).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

PAD_ID = np.iinfo(np.uint64).max
BIG_DIST = np.float32(3.402823e38)


def as_set(X) -> frozenset:
    return frozenset(int(x) for x in np.asarray(X, dtype=np.int64).reshape(-1))


def _padded(ids, dists, k):
    out_i = np.full(k, PAD_ID, np.uint64)
    out_d = np.full(k, BIG_DIST, np.float32)
    n = min(k, len(ids))
    out_i[:n] = ids[:n]
    out_d[:n] = dists[:n]
    return out_i, out_d


def masked_rerank(ix, q, log, cnt, X, k, mips=False):
    """One query: the re-rank (K6 + K7) of log[:cnt] without its entries in X.  -> (ids u64 [k], dists f32 [k])"""
    X = as_set(X)
    orc = O.Oracle(ix)
    live = np.array([int(x) for x in np.asarray(log)[:int(cnt)] if int(x) not in X], np.uint32)
    if len(live) == 0:
        return _padded([], [], k)
    d = np.array([orc.exact_dist(int(x), q, 1 if mips else 0) for x in live], np.float32)
    kk = min(k, len(live))
    ids, dists = O.topk(live, d, kk)
    return _padded(ids, dists, k)


def masked_worklist(ids_L, dists_L, X, k):
    """One query: ids_L u64 [L] / dists_L f32 [L] are the reference's results at k = L (the final worklist, padded).  -> (ids [k], dists [k])"""
    X = as_set(X)
    keep_i, keep_d = [], []
    for x, d in zip(np.asarray(ids_L, np.uint64), np.asarray(dists_L, np.float32)):
        if int(x) == int(PAD_ID):
            break
        if int(x) in X:
            continue
        keep_i.append(x)
        keep_d.append(d)
    return _padded(keep_i, keep_d, k)


# ---- the walks: logs and counters of the unmasked references ----------------------------------------------------------------------------
def walk_base(ix, queries, k, L, layout="split", mips=False):
    """BANG_Base walk (layout "split") or the word-local filter ("word"): -> (ids, dists, stats, log [Q][L + 50], counts)"""
    from wordfilter_reference import Reference
    ref = Reference(ix)
    Q = queries.shape[0]
    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((k, Q), np.float32)
    st = np.empty((Q, 4), np.int64)
    logs = np.zeros((Q, L + 50), np.uint32)
    cnt = np.zeros(Q, np.uint32)
    for i in range(Q):
        lg = []
        ids[i], dists[:, i], st[i] = ref.search_one(queries[i], k, L, layout, mips, log=lg)
        logs[i, :len(lg)] = lg
        cnt[i] = len(lg)
    return ids, dists, st, logs, cnt


def walk_inmemory(ix, queries, k, L):
    """semantics = 1: -> (ids, dists, stats, log [Q][L + 120], counts)"""
    from inmemory_reference import Reference
    ref = Reference(ix)
    Q = queries.shape[0]
    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((k, Q), np.float32)
    st = np.empty((Q, 4), np.int64)
    logs = np.zeros((Q, L + 120), np.uint32)
    cnt = np.zeros(Q, np.uint32)
    for i in range(Q):
        ids[i], dists[:, i], st[i], c = ref.search_one_logged(queries[i], k, L, "inmemory")
        logs[i, :len(c)] = c
        cnt[i] = len(c)
    return ids, dists, st, logs, cnt


def walk_exact(ix, queries, L, beam=1):
    """distance = 1 at k = L: -> (ids u64 [Q][L], dists f32 [L][Q], stats); beam = 1 is exact_reference's walk, 2..4 beam_reference's"""
    if beam > 1:
        from beam_reference import Reference
        ids, dists, st, _ = Reference(ix).search(queries, L, L, beam)
        return ids, dists, st
    from exact_reference import Reference
    return Reference(ix).search(queries, L, L, "exact")


def rerank_all(ix, queries, logs, cnt, X, k, mips=False):
    Q = queries.shape[0]
    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((k, Q), np.float32)
    for i in range(Q):
        ids[i], dists[:, i] = masked_rerank(ix, queries[i], logs[i], cnt[i], X, k, mips)
    return ids, dists


def worklist_all(ids_L, dists_L, X, k):
    Q = ids_L.shape[0]
    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((k, Q), np.float32)
    for i in range(Q):
        ids[i], dists[:, i] = masked_worklist(ids_L[i], dists_L[:, i], X, k)
    return ids, dists


# ---- the masks of tests/test_gpu_exclude.py (fixed seed) -------------------------------------------------------------------------------
MASKS = ("rand30", "top", "edges", "all_but_one")


def make_mask(name, ix, rank0=None, seed=1234):
    """rank0: the rank-0 result ids of the unmasked run over all queries (mask "top")."""
    N = int(ix.N)
    if name == "none":
        return np.zeros(0, np.uint32)
    if name == "rand30":
        return np.sort(np.random.default_rng(seed).choice(N, size=(N * 3) // 10, replace=False)).astype(np.uint32)
    if name == "top":
        r = np.asarray(rank0, np.uint64).reshape(-1)
        return np.unique(r[r != PAD_ID]).astype(np.uint32)
    if name == "edges":
        return np.unique(np.array([0, 31, 32, N - 1, int(ix.medoid)], np.uint32))
    if name == "all_but_one":
        keep = int(np.random.default_rng(seed).integers(0, N))
        return np.array([i for i in range(N) if i != keep], np.uint32)
    raise ValueError(name)
