"""Inputs of the insert tests: small indexes in the shapes of the conftest fixtures and the batches inserted into them.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_insert_reference.py asserts ON THE CPU REFERENCE that these inputs reach the
edges (rows that end short of R and rows that stop full, both back-edge paths, a changed medoid row, a target with >= 3 incoming ids, a candidate
at distance 0); tests/test_gpu_insert.py runs them on the GPU.

    INDEXES, get()     synth.make_index(device="cpu") per layout: int8 D=64 R=32 m=16 N=2000; uint8 D=128 R=64 m=70 N=4000; float D=96 m=74 N=2500;
                       float D=128 m=32 N=3000
    batch()            16 .. 96 points: perturbed copies of indexed vectors, four exact duplicates of indexed vectors, one copy of the medoid's vector
    CASES              (index, batch size, L_build, alpha, seed) of every engine case; reference() = insert_reference.insert on it, computed once
"""
from __future__ import annotations

import functools

import numpy as np

from bang_amd import synth
from bang_amd.binding import NP_DTYPE

# name -> (N, D, dtype, R, m, Q, seed): the shapes of conftest's small_i8, small_u8, small_deep, small_f32
INDEXES = {
    "i8":   (2000, 64, "int8", 32, 16, 32, 14),
    "u8":   (4000, 128, "uint8", 64, 70, 64, 12),
    "deep": (2500, 96, "float", 64, 74, 40, 13),
    "f32":  (3000, 128, "float", 64, 32, 48, 11),
}

# name -> (index, n, L_build, alpha, seed)
CASES = {
    "i8_a12":   ("i8", 48, 40, 1.2, 1),
    "i8_a8":    ("i8", 16, 64, 8.0, 2),      # L_build > R = 32 at alpha = 8: every new row stops full
    "u8_a12":   ("u8", 96, 64, 1.2, 3),
    "u8_a8":    ("u8", 16, 100, 8.0, 4),     # L_build > R = 64
    "deep_a12": ("deep", 64, 48, 1.2, 5),
    "f32_a12":  ("f32", 32, 72, 1.2, 6),
}
SECOND = ("i8", 24, 40, 1.2, 7)              # the batch that follows "i8_a12" in the two-batch test


@functools.lru_cache(maxsize=None)
def get(name: str):
    """-> (Index, queries [Q][D]); treat both as read-only."""
    N, D, dtype, R, m, Q, seed = INDEXES[name]
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=32, seed=seed, device="cpu", pq_iters=4)
    return ix, np.ascontiguousarray(q)


def batch(ix, n: int, seed: int) -> np.ndarray:
    """n new vectors of ix's type: n - 5 perturbed copies of indexed vectors, four exact duplicates of indexed vectors, the medoid's vector."""
    assert n >= 16
    rng = np.random.default_rng(4200 + seed)
    base = ix.vectors()
    pick = rng.choice(ix.N, n, replace=False)
    v = base[pick].astype(np.float64)
    if ix.dtype == "float":
        v = v + rng.standard_normal(v.shape) * 0.05 * base.astype(np.float64).std()
        out = v.astype(np.float32)
    else:
        info = np.iinfo(NP_DTYPE[ix.dtype])
        out = np.clip(np.rint(v + rng.integers(-3, 4, v.shape)), info.min, info.max).astype(NP_DTYPE[ix.dtype])
    out[n - 5: n - 1] = base[pick[n - 5: n - 1]]                         # four exact duplicates
    out[n - 1] = base[ix.medoid]                                         # the medoid's vector
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (Index, vectors, L_build, alpha)"""
    iname, n, L, alpha, seed = CASES[name]
    ix, _ = get(iname)
    return ix, batch(ix, n, seed), L, alpha


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """-> (Index', stats) of insert_reference.insert on the case; computed once, treat as read-only."""
    import insert_reference
    ix, v, L, alpha = case(name)
    return insert_reference.insert(ix, v, L, alpha)


DUP = ("i8", 500, 40, 1.2, 7)                # 500 copies of indexed vector 7: node 7 is in every new row, 64 + 500 candidates meet the cap of 512


@functools.lru_cache(maxsize=None)
def dup_reference():
    """-> (Index, vectors, L_build, alpha, Index', stats) of the batch whose back-edges overflow the 512-entry candidate list of one target"""
    import insert_reference
    iname, n, L, alpha, node = DUP
    ix, _ = get(iname)
    v = np.ascontiguousarray(np.repeat(ix.vectors()[node:node + 1], n, axis=0))
    return (ix, v, L, alpha) + insert_reference.insert(ix, v, L, alpha)


@functools.lru_cache(maxsize=None)
def second_reference():
    """the reference applied twice: SECOND's batch into the Index' of "i8_a12" -> (vectors of the second batch, Index'', stats)"""
    import insert_reference
    ix1, _ = reference("i8_a12")
    _, n, L, alpha, seed = SECOND
    v = batch(ix1, n, seed)
    ix2, st = insert_reference.insert(ix1, v, L, alpha)
    return v, ix2, st
