"""The index of tests/test_gpu_rows_pad.py: the smallest on which every source of an adjacency row is read and every seam between them is crossed.

uint8, D = 128, m = 70 (the <2, 18> layout: code rows 128 bytes apart, 14 ids of padding per line), N = 1003 -- not a multiple of the 5 lines a
padded row takes, so n_pad = 200 and the lines 1000 .. 1002 hold none -- R = 64, 64 queries, L = 37, k = 10.  With BANG_ROWS_HBM_MAX_ROWS = 256 the
rows of the nodes [0, 200) sit in the padding, [200, 456) in the HBM copy, [456, 1003) are pulled: the SEAMS 199 | 200 and 455 | 456.

synth.make_index's graph, changed so that the seams are walked whatever the data: seam node s takes the vector and the code row of the nearest
neighbour of query j (so it is among the closest nodes of that query and is expanded once it is in the worklist), and the medoid's row -- the seed
list of every query -- lists the four seam nodes first.  Their rows have the degrees 1, 13, 14 and 15 (one id, one short of a line's 14 slots, a full
line, one more); the medoid's row has 64."""
import dataclasses
import functools

import numpy as np

N, D, M, R, Q, L, K = 1003, 128, 70, 64, 64, 37, 10
N_PAD, N_COPY = 200, 256
SEAMS = (199, 200, 455, 456)
DEGREES = {199: 1, 200: 13, 455: 14, 456: 15}


@functools.lru_cache(maxsize=None)
def index():
    """-> (ix, queries [700][D]: the 64 of the synthetic index and 636 more made of them)"""
    from bang_amd import formats, synth
    ix, q, gt_i, _ = synth.make_index(N, D, "uint8", R, M, Q, K=K, n_clusters=32, seed=21, device="cpu", pq_iters=4)
    vec, deg, adj, codes = ix.vectors(), ix.degrees().copy(), ix.adjacency().copy(), ix.codes.copy()
    med = int(ix.medoid)
    assert med not in SEAMS and deg[med] >= 8
    for j, s in enumerate(SEAMS):
        g = int(gt_i[j, 0])
        assert g not in SEAMS
        vec[s], codes[s] = vec[g], codes[g]
    for s, d in DEGREES.items():
        assert deg[s] >= d
        deg[s] = d
    own = [int(x) for x in adj[med][:deg[med]] if int(x) not in SEAMS]
    more = [x for x in range(N) if x != med and x not in SEAMS and x not in own]
    adj[med] = np.array((list(SEAMS) + own + more)[:R], np.uint32)
    deg[med] = R
    ix = dataclasses.replace(ix, graph=formats.pack_graph(vec, deg, adj), codes=codes)
    rng = np.random.default_rng(5)
    extra = q[rng.integers(0, Q, 700 - Q)].astype(np.int64) + rng.integers(-3, 4, (700 - Q, D))
    return ix, np.concatenate([q, np.clip(extra, 0, 255).astype(np.uint8)])


@functools.lru_cache(maxsize=None)
def reference(n_queries: int):
    """the oracle's answer for the first n_queries queries, computed once: (ids, dists, stats [Q][4] {iterations, candidates, evaluations, fetched})"""
    from oracle import oracle as O
    ix, q = index()
    return O.Oracle(ix).search(q[:n_queries], K, L, with_stats=True)


def padded_table(codes: np.ndarray, rows: np.ndarray, n_pad: int, fill: int = 0) -> np.ndarray:
    """[N][128] code lines (m = 70) as the load lays them out: the code bytes, `fill` behind them, and the ids of the rows [0, n_pad) in the bytes
    72 .. 127 of their 5 lines (14 per line; the slots behind the 64th id 0xFFFFFFFF) -- csrc/bang_pad_rows.h restated"""
    n = codes.shape[0]
    t = np.full((n, 128), fill, np.uint8)
    t[:, :codes.shape[1]] = codes
    pad = t[:, 72:].view(np.uint32)                      # [N][14]
    for r in range(n_pad):
        ids = np.full(70, 0xFFFFFFFF, np.uint32)
        ids[:64] = rows[r]
        pad[5 * r:5 * r + 5] = ids.reshape(5, 14)
    return t
