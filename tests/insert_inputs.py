"""Inputs of the insert tests: small indexes in the shapes of the conftest fixtures and the batches inserted into them.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_insert_reference.py asserts ON THE CPU REFERENCE that these inputs reach the
edges (rows that end short of R and rows that stop full, both back-edge paths, a changed medoid row, a target with >= 3 incoming ids, a candidate
at distance 0); tests/test_gpu_insert.py runs them on the GPU.

    INDEXES, get()     synth.make_index(device="cpu") per layout: int8 D=64 R=32 m=16 N=2000; uint8 D=128 R=64 m=70 N=4000; float D=96 m=74 N=2500;
                       float D=128 m=32 N=3000
    batch()            16 .. 96 points: perturbed copies of indexed vectors, four exact duplicates of indexed vectors, one copy of the medoid's vector
    CASES              (index, batch size, L_build, alpha, seed) of every engine case; reference() = insert_reference.insert on it, computed once
    SEAMS              the chunk sizes (test hooks) under which a case crosses the seams of bang_insert_e; DUP_MIXED: 500 copies ++ 40 distinct points
    LAYOUTS, layout()  N = 300, R = 16 indexes at the vector layouts INDEXES leaves out
    LATTICES           300 integer lattice points in the layout of "i8" / "u8": tie-rich lists for the kill rule
    PQ_LAYOUTS         pivot tables of m = 1 .. 129 chunks with equal rows (PQ_TIES) for the arg-min
    FORM_CASES         the cases every search form runs on after the insert, form_queries() their 24 queries
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


# ---------------------------------------------------------------------------------------------------------------------
# chunk seams (environment test hooks BANG_INSERT_SEARCH_CHUNK / _TARGET_CHUNK / _ENCODE_CHUNK)
# ---------------------------------------------------------------------------------------------------------------------
# case -> (search chunk, target chunk, encode chunk); None = the engine's own size.  The reference knows no chunks: the results are reference()'s
SEAMS = {
    "i8_a12":    (20, 64, 7),        # 48 points: 20 + 20 + 8
    "u8_a12":    (33, 100, 50),      # 96 points
    "deep_a12":  (1, 1, 1),
    "DUP_MIXED": (128, 16, 96),      # 540 points; the last search chunk (512 ..) and the last encode chunk (480 ..) hold the 40 distinct vectors
}
DUP_MIXED_TAIL = 40


@functools.lru_cache(maxsize=None)
def dup_mixed_reference():
    """DUP's 500 copies followed by batch(ix, 40, 7): rows and codes behind the search and encode seams differ from those in front.  (Replacing
    the last 40 of the 500 copies instead would leave R + 460 = 492 candidates per target: under the cap of 512, nothing dropped.)
    -> (Index, vectors, L_build, alpha, Index', stats)"""
    import insert_reference
    iname, n, L, alpha, node = DUP
    ix, _ = get(iname)
    v = np.ascontiguousarray(np.concatenate([np.repeat(ix.vectors()[node:node + 1], n, axis=0), batch(ix, DUP_MIXED_TAIL, node)]))
    return (ix, v, L, alpha) + insert_reference.insert(ix, v, L, alpha)


def seam_case(name: str):
    """-> (Index, vectors, L_build, alpha, Index', stats) of a SEAMS case"""
    if name == "DUP_MIXED":
        return dup_mixed_reference()
    return case(name) + reference(name)


# ---------------------------------------------------------------------------------------------------------------------
# every vector layout of bang_search_can_rerank the four INDEXES leave out: G = 1, 2, 16; float D = 4, a partly filled third register (D = 160),
# a partly filled fourth (D = 200), four full ones
# ---------------------------------------------------------------------------------------------------------------------
# name -> (D, dtype, m); N = 300, R = 16, two k-means rounds: cheap to build
LAYOUTS = {
    "u8_16":   (16, "uint8", 8),
    "i8_32":   (32, "int8", 8),
    "u8_256":  (256, "uint8", 16),
    "f32_4":   (4, "float", 2),
    "f32_160": (160, "float", 8),
    "f32_200": (200, "float", 8),
    "f32_256": (256, "float", 16),
}
LAYOUT_N, LAYOUT_R = 300, 16


@functools.lru_cache(maxsize=None)
def layout(name: str):
    """-> Index of a LAYOUTS entry; read-only."""
    D, dtype, m = LAYOUTS[name]
    ix, _, _, _ = synth.make_index(LAYOUT_N, D, dtype, LAYOUT_R, m, 4, K=10, n_clusters=8, seed=40 + D, device="cpu", pq_iters=2)
    return ix


def make_list(ref, rng, node: int, length: int, pool: int | None = None):
    """An ordered candidate list of `length` distinct ids around `node`: ascending exact distance to its vector, as a worklist is."""
    import insert_reference
    pool = ref.ix.N if pool is None else pool
    ids = rng.choice(pool, length, replace=False).astype(np.uint32)
    d = ref.exact(ids, insert_reference.vector_of(ref, node))
    o = np.argsort(d, kind="stable")
    return ids[o], d[o]


# ---------------------------------------------------------------------------------------------------------------------
# tie-rich indexes: 300 distinct points of a small integer lattice in the first dimensions, zero elsewhere.  Squared distances are small integers.
#   "tern6":  {0, 1, 2}^6 -- e == d_t (alpha = 1) is common: '<=' and '<' give different rows
#   "plane7": {0 .. 6}^2 x {0, 1}^3 -- holds e = 25 with d_t = 36 and e = 50 with d_t = 72: fl32(1.44f * 25) = 36 and fl32(1.44f * 50) = 72 exactly,
#             while the unrounded products lie above (1.44f = 1.440000057...): the rounding of the one float32 multiply decides the kill
# ---------------------------------------------------------------------------------------------------------------------
LATTICES = {"tern6": (3, 3, 3, 3, 3, 3), "plane7": (7, 7, 2, 2, 2)}
LATTICE_N = 300
LATTICE_LENGTHS = (64, 65, 300)


@functools.lru_cache(maxsize=None)
def lattice(iname: str, kind: str = "tern6"):
    """-> Index in the layout of INDEXES[iname] ("i8": D = 64, "u8": D = 128) whose 300 vectors are distinct lattice points; rows empty."""
    import dataclasses
    from bang_amd import formats
    ix, _ = get(iname)
    bases = LATTICES[kind]
    rng = np.random.default_rng(600)
    pick = np.sort(rng.choice(int(np.prod(bases)), LATTICE_N, replace=False))
    v = np.zeros((LATTICE_N, ix.D), NP_DTYPE[ix.dtype])
    for k, b in enumerate(bases):
        v[:, k] = pick % b
        pick = pick // b
    graph = formats.pack_graph(v, np.zeros(LATTICE_N, np.uint32), np.zeros((LATTICE_N, ix.R), np.uint32))
    return dataclasses.replace(ix, N=LATTICE_N, medoid=0, graph=graph, codes=np.zeros((LATTICE_N, ix.m), np.uint8))


@functools.lru_cache(maxsize=None)
def lattice_lists(iname: str, kind: str = "tern6"):
    """-> (lists, owns): four lists of each of LATTICE_LENGTHS around random lattice points; the 300-entry lists hold their own node"""
    from exact_reference import Reference
    ref = Reference(lattice(iname, kind))
    rng = np.random.default_rng(77)
    lists, owns = [], []
    for length in LATTICE_LENGTHS:
        for _ in range(4):
            node = int(rng.integers(LATTICE_N))
            lists.append(make_list(ref, rng, node, length))
            owns.append(node)
    return lists, owns


# ---------------------------------------------------------------------------------------------------------------------
# PQ layouts for pq_argmin_kernel: no graph is needed, the oracle's lut_build is the reference
# ---------------------------------------------------------------------------------------------------------------------
# name -> (m, D): one chunk; exactly one pass of 64 chunks; a pass and a tail of one; two passes; two passes and a tail of one
PQ_LAYOUTS = {"m1": (1, 16), "m64": (64, 64), "m65": (65, 130), "m128": (128, 128), "m129": (129, 258)}
# (lower k, higher k) of the pivot rows made equal: the same lane (k, k + 64: the lane's strict '<'); the lower k in the HIGHER lane (70 -> lane 6,
# 133 -> lane 5: the second key word of the wave's minimum); the ends
PQ_TIES = ((3, 67), (70, 133), (0, 255))


@functools.lru_cache(maxsize=None)
def pq_layout(name: str):
    """-> (Index, vectors [9][D] float32): random pivots with the PQ_TIES rows copied; vectors 0 .. 2 are centroid + the tied pivot (the tied pair
    is at distance 0 of every chunk: the row minimum), the rest are random."""
    from bang_amd import formats
    m, D = PQ_LAYOUTS[name]
    rng = np.random.default_rng(900 + m)
    piv = rng.standard_normal((256, D)).astype(np.float32)
    for lo, hi in PQ_TIES:
        piv[hi] = piv[lo]
    cen = rng.standard_normal(D).astype(np.float32)
    v = rng.standard_normal((9, D)).astype(np.float32)
    for i, (lo, _) in enumerate(PQ_TIES):
        v[i] = piv[lo] + cen
    graph = formats.pack_graph(np.zeros((1, D), np.float32), np.zeros(1, np.uint32), np.zeros((1, 4), np.uint32))
    ix = formats.Index(dtype="float", N=1, D=D, R=4, m=m, medoid=0, graph=graph, codes=np.zeros((1, m), np.uint8), pivots=piv, centroid=cen,
                       chunk_off=synth.chunk_offsets(D, m))
    return ix, np.ascontiguousarray(v)


# ---------------------------------------------------------------------------------------------------------------------
# every search form after an insert
# ---------------------------------------------------------------------------------------------------------------------
FORM_CASES = ("i8_a12", "f32_a12", "u8_a12")


def form_queries(name: str) -> np.ndarray:
    """24 queries of a FORM_CASES case: 16 of the index's queries and 8 of the inserted vectors"""
    _, v, _, _ = case(name)
    return np.ascontiguousarray(np.concatenate([get(CASES[name][0])[1][:16], v[:8]]))
