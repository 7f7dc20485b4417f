"""Small deterministic indexes with the wide vector layouts of the exact-distance search mode: D up to 1024, 8-bit vectors whose D / 16
is not a power of two, and 8-bit distances past 2^24 (where orc_exact_dist's float chain rounds and the integer sum is not its value).

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_highdim_inputs.py asserts ON THE CPU REFERENCE that every input
reaches the ground it is named for; tests/test_gpu_exact_highdim.py compares the kernel with that reference bit for bit.

    gist_like    float  D = 960   N 3000  R 32  m 120  Q 24     the GIST1M layout
    mnist_like   uint8  D = 784   N 3000  R 32  m 98   Q 24     the MNIST8M layout: D / 16 = 49
    i8_1024      int8   D = 1024  N 2000  R 24  m 64   Q 16     the widest layout
    u8_48        uint8  D = 48    N 2000  R 24  m 12   Q 16     D / 16 = 3
    f32_260      float  D = 260   N 600   R 32  m 65   Q 12     the first float layout past 256: a fifth query register
    far_u8       uint8  D = 784   mnist_like's graph, base bytes in [0, 40), query bytes in [216, 256): every distance > 2^24
    far_i8       int8   D = 1024  i8_1024's graph, base in [-128, -90), queries in [90, 128): every distance > 2^24
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from bang_amd import synth
from bang_amd.formats import NP_DTYPE, pack_graph

TWO24 = 1 << 24

# name -> (N, D, dtype, R, m, Q)
SYNTH = {
    "gist_like":  (3000, 960,  "float", 32, 120, 24),
    "mnist_like": (3000, 784,  "uint8", 32, 98,  24),
    "i8_1024":    (2000, 1024, "int8",  24, 64,  16),
    "u8_48":      (2000, 48,   "uint8", 24, 12,  16),
    "f32_260":    (600,  260,  "float", 32, 65,  12),
}
# name -> (the input whose graph it keeps, base range, query range): half-open integer ranges
FAR = {
    "far_u8": ("mnist_like", (0, 40), (216, 256)),
    "far_i8": ("i8_1024", (-128, -90), (90, 128)),
}
NAMES = tuple(SYNTH) + tuple(FAR)
LS = (10, 37, 152)


@functools.lru_cache(maxsize=None)
def get(name: str):
    """-> (Index, queries [Q][D])"""
    if name in SYNTH:
        N, D, dtype, R, m, Q = SYNTH[name]
        ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=8, seed=3000 + D + R, device="cpu", pq_iters=2)
        return ix, q
    src, (blo, bhi), (qlo, qhi) = FAR[name]
    ix, q = get(src)
    rng = np.random.default_rng(4000 + ix.D)
    vec = rng.integers(blo, bhi, (ix.N, ix.D)).astype(NP_DTYPE[ix.dtype])
    qq = rng.integers(qlo, qhi, q.shape).astype(NP_DTYPE[ix.dtype])
    # (the PQ side of the index is left as it is: these two inputs are for the exact mode only)
    return dataclasses.replace(ix, graph=pack_graph(vec, ix.degrees(), ix.adjacency())), np.ascontiguousarray(qq)


def integer_sums(ix, ids: np.ndarray, query: np.ndarray) -> np.ndarray:
    """int64: sum over the dimensions of (vector - query)^2 for 8-bit vectors, exact."""
    v = ix.vectors()[np.asarray(ids, np.int64)].astype(np.int64)
    d = v - query.astype(np.int64)[None, :]
    return (d * d).sum(axis=1)
