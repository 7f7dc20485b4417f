"""Small deterministic indexes that drive the search kernels to their edges.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  The fixtures of tests/conftest.py never reach these places (exact distance
ties, the 65-id seed list, the iteration cap, a worklist shorter than k, the vector layouts at either end of what the kernels evaluate,
values at the ends of the 8-bit ranges); every input here is named for the edge it reaches, tests/test_edge_inputs.py asserts ON THE CPU
REFERENCES that it does reach it, and the GPU files compare the kernels with those references bit for bit: tests/test_gpu_exact_edges.py and
tests/test_gpu_exact_pull.py (the exact-distance kernels), tests/test_gpu_inmemory_edges.py (the Inmemory build), tests/test_gpu_lut_search.py
(the LUT-path kernel) and tests/test_gpu_base_edges.py (every form of the BANG_Base PQ walk; the forms are those of tests/base_forms.py).
The layout list that reaches every compiled instance of that walk's kernel, in both row alignments, is a module of its own:
tests/instance_inputs.py, asserted by tests/test_instance_inputs.py and run by tests/test_gpu_search_instances.py.

    (a) toy(), TOYS               hand-made graphs with level vectors (inmemory_reference.toy_index) in any vector type and dimension
    (b) chain()                   a chain with a falling distance: the walk runs to the iteration cap
    (c) short_worklist()          three nodes, a self-loop and a duplicate id: the worklist stays shorter than k
    (d) seed65()                  a medoid of degree R = 64: a seed list of 65 ids, the 65th best / tying the best / worse
        degree64()                the first parent has 64 neighbours: a row without a pad
    (e) tie_heavy()               a fixture with its vectors, queries and pivots cut down to a few small integers: ties everywhere
    (f) extreme()                 8-bit vectors of the two end values at D = 256: distances just below 2^24
    (g) SHAPES, shape_index()     synth.make_index at the dimensions and degree bounds at the ends of the supported layouts
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from bang_amd import synth
from bang_amd.formats import NP_DTYPE, pack_graph
from inmemory_reference import toy_index

ID_PAD = np.iinfo(np.uint64).max


# ---------------------------------------------------------------------------------------------------------------------
# (a) toy graphs in any vector type and dimension
# ---------------------------------------------------------------------------------------------------------------------
def toy(adj: dict, levels: list, dtype: str = "uint8", D: int = 128, medoid: int = 0, R: int = 64, query_level: int = 0):
    """inmemory_reference.toy_index with the vector type and the dimension chosen.  Levels count from the low end of the type's range
    (lo = -128 for int8, else 0): node i's vector is lo + levels[i] in every dimension, the query lo + query_level -- an int8 index has the
    differences of the uint8 one, from operands of both signs.  PQ: chunks of 4 dimensions (m = D / 4), pivot c is lo + c in every
    dimension, node i's codes are levels[i] and the centroid is 0 -- so the PQ distance of node i equals its exact distance,
    D (levels[i] - query_level)^2, an integer below 2^24 that float arithmetic gives exactly in any order.  Equal levels are exact ties."""
    assert D % 4 == 0 and D * 255 * 255 < (1 << 24)
    base, _ = toy_index(adj, levels, medoid=medoid, R=R)                           # (the adjacency and the codes' values)
    lo = -128 if dtype == "int8" else 0
    lv = np.asarray(levels, np.int64)
    assert lv.min() >= 0 and lv.max() <= 255 and 0 <= query_level <= 255
    vec = np.repeat(lo + lv[:, None], D, axis=1).astype(NP_DTYPE[dtype])
    m = D // 4
    ix = dataclasses.replace(
        base, dtype=dtype, D=D, m=m, graph=pack_graph(vec, base.degrees(), base.adjacency()),
        codes=np.repeat(lv.astype(np.uint8)[:, None], m, axis=1).copy(),
        pivots=np.repeat((np.arange(256) + lo).astype(np.float32)[:, None], D, axis=1),
        centroid=np.zeros(D, np.float32), chunk_off=np.arange(0, D + 1, 4, dtype=np.uint32))
    return ix, np.full((1, D), lo + query_level, NP_DTYPE[dtype])


# name -> (adjacency, levels): the three walks of tests/inmemory_reference.py, and a tie between the best survivor and the worklist's head
# whose two nodes lead to different places (the kernel's strict `bd < head.d`: the worklist entry is expanded first)
TOYS = {
    "tie":        ({0: [1, 2], 1: [3], 2: [4], 3: [5]}, [200, 10, 20, 20, 5, 6]),
    "not_full":   ({0: [1], 1: [2], 2: [3]}, [50, 10, 100, 1]),
    "medoid_tie": ({0: [1, 2], 1: [3], 2: [4]}, [10, 10, 20, 5, 6]),
    "head_tie":   ({0: [1, 2, 3], 1: [4], 2: [5], 3: [6], 4: [7], 5: [8]}, [120, 30, 40, 50, 40, 9, 8, 7, 3]),
}
TOY_LAYOUTS = (("uint8", 16), ("uint8", 128), ("int8", 64), ("int8", 256), ("float", 20), ("float", 128))


def toy_named(name: str, dtype: str, D: int):
    adj, levels = TOYS[name]
    return toy(adj, levels, dtype, D)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the iteration cap
# ---------------------------------------------------------------------------------------------------------------------
def chain(dtype: str = "uint8", D: int = 128, n: int = 256):
    """0 -> 1 -> ... -> n - 1 with the distance falling strictly along the chain (inmemory_reference.chain_index in any layout): every
    iteration has one survivor, better than everything before it, and the walk only ends at the iteration cap."""
    return toy({i: [i + 1] for i in range(n - 1)}, [255 - i for i in range(n)], dtype, D)


# ---------------------------------------------------------------------------------------------------------------------
# (c) a worklist shorter than k
# ---------------------------------------------------------------------------------------------------------------------
def short_worklist(dtype: str = "uint8", D: int = 128):
    """Three nodes; node 1's row holds itself and node 2 twice.  Every id is in the filter after iteration 1, so nothing more survives:
    the worklist ends with three entries and a search with k = 10 pads seven (CANON 8)."""
    return toy({0: [1, 2], 1: [1, 2, 2], 2: [0]}, [30, 10, 20], dtype, D)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the 65-id seed list
# ---------------------------------------------------------------------------------------------------------------------
SEED65_VARIANTS = ("best", "tie", "worse")
SEED65_LAYOUTS = (("uint8", 128), ("int8", 64), ("float", 128))
SEED65_BEST_OF_64 = 3            # the first of the two equal minima among seed ids 0 .. 63
SEED65_LAST = 64                 # the 65th seed id


def seed65(dtype: str, variant: str, D: int = 128):
    """Medoid 0 with R = 64 neighbours 1 .. 64: the seed list [medoid, 1, ..., 64] has 65 ids, and node 64 is the one element a wave's 64
    lanes do not hold.  Among the first 64 ids, nodes 3 and 7 tie for the minimum (level 20; the first one wins); node 64 is strictly better
    (level 10), ties them (20) or is worse (30).  Nodes 3, 7 and 64 lead to different, ever better nodes, so the order in which they are
    expanded shows in the worklist at small L."""
    level64 = {"best": 10, "tie": 20, "worse": 30}[variant]
    levels = [100] + [40 + (i * 7) % 23 for i in range(1, 64)] + [level64]
    levels[3] = levels[7] = 20
    adj = {0: list(range(1, 65)), 3: [65, 66], 7: [67, 68], 64: [69, 70], 1: [71], 65: [72], 67: [73], 69: [74], 72: [75]}
    levels += [9, 16, 8, 15, 6, 12, 35, 5, 4, 3, 2]                                # nodes 65 .. 75
    assert len(levels) == 76
    return toy(adj, levels, dtype, D)


# ---------------------------------------------------------------------------------------------------------------------
# (d2) an expanded row of 64 ids
# ---------------------------------------------------------------------------------------------------------------------
DEGREE64_LAYOUTS = (("uint8", 128), ("float", 128))
DEGREE64_NODE = 1                # the first parent


def degree64(dtype: str = "uint8", D: int = 128):
    """Node 1 is the first parent and has exactly 64 neighbours: its 256-byte row holds no pad and all 64 lanes carry an id."""
    levels = [200, 100] + [50 + (i * 5) % 41 for i in range(64)] + [7, 3]
    adj = {0: [1], 1: list(range(2, 66)), 2: [66], 66: [67]}
    return toy(adj, levels, dtype, D)


# ---------------------------------------------------------------------------------------------------------------------
# (e) ties everywhere
# ---------------------------------------------------------------------------------------------------------------------
def tie_heavy(ix, q, n_queries: int = 16):
    """A fixture (conftest.small_u8 / small_i8 / small_f32 / small_deep) with the same adjacency and every value cut down to a few small
    integers: 8-bit vectors and queries shifted right by 6 bits (uint8 0 .. 3, int8 -2 .. 1), float ones doubled and rounded (about -3 .. 3).
    The distances are small integers -- exact in float -- and most of a query's nearest nodes tie.  The pivots get the same treatment
    (pivot + centroid, cut down the same way, centroid 0; the codes stay), so the PQ distances tie as well."""
    if ix.dtype == "float":
        cut = lambda a: np.rint(np.asarray(a, np.float32) * 2.0).astype(np.float32)          # noqa: E731
    else:
        cut = lambda a: np.floor(np.asarray(a, np.float32) / 64.0).astype(np.float32)         # noqa: E731  (>> 6, arithmetic)
    vec = cut(ix.vectors()).astype(NP_DTYPE[ix.dtype])
    ix2 = dataclasses.replace(ix, graph=pack_graph(vec, ix.degrees(), ix.adjacency()), pivots=cut(ix.pivots + ix.centroid[None, :]),
                              centroid=np.zeros(ix.D, np.float32))
    return ix2, np.ascontiguousarray(cut(q[:n_queries]).astype(NP_DTYPE[ix.dtype]))


# ---------------------------------------------------------------------------------------------------------------------
# (f) the ends of the 8-bit ranges at D = 256
# ---------------------------------------------------------------------------------------------------------------------
def extreme(dtype: str, N: int = 160, Q: int = 8, R: int = 32, seed: int = 7):
    """uint8 vectors of {0, 255} / int8 vectors of {-128, 127} at D = 256: a node at one end against a query at the other is
    256 x 255^2 = 16 646 400 away, just below 2^24, the largest integer distance the kernels' integer identity has to carry into float.
    Node i has i mod 11 of its dimensions at the low end (nodes 0, 11, ... are all high), node 1 is all low; the queries are all low,
    all high, and the same with a few dimensions flipped.  Graph: a ring plus random links, degrees ragged.  PQ: chunks of 4 dimensions,
    pivot c < 16 spells the 16 patterns of {low, high}^4, so the PQ distance is the exact one."""
    assert dtype in ("uint8", "int8")
    D, m = 256, 64
    lo, hi = (0, 255) if dtype == "uint8" else (-128, 127)
    rng = np.random.default_rng(seed)
    bits = np.ones((N, D), np.uint8)                                               # 1 = high
    for i in range(N):
        bits[i, rng.permutation(D)[: i % 11]] = 0
    bits[1] = 0
    bits[2::7] = rng.integers(0, 2, (len(range(2, N, 7)), D), dtype=np.uint8)      # some nodes in the middle
    qbits = np.zeros((Q, D), np.uint8)
    qbits[1::2] = 1
    for j in range(2, Q):
        qbits[j, rng.permutation(D)[: j]] ^= 1
    deg = np.zeros(N, np.uint32)
    nbr = np.zeros((N, R), np.uint32)
    for i in range(N):
        row = set(rng.integers(0, N, rng.integers(3, R)).tolist()) | {(i + 1) % N}
        row.discard(i)
        row = sorted(row)[:R]
        deg[i] = len(row)
        nbr[i, :len(row)] = row
    pat = (np.arange(256)[:, None] >> np.arange(4)[None, :]) & 1                    # pivot c, dimension j of a chunk: bit j of c
    pivots = np.where(np.tile(pat, (1, m)) == 1, hi, lo).astype(np.float32)         # [256][D]
    codes = (bits.reshape(N, m, 4) << np.arange(4, dtype=np.uint8)[None, None, :]).sum(axis=2).astype(np.uint8)
    val = lambda b: np.where(b == 1, hi, lo).astype(NP_DTYPE[dtype])                # noqa: E731
    base, _ = toy_index({}, [0] * N, medoid=0, R=R)
    ix = dataclasses.replace(base, dtype=dtype, D=D, m=m, graph=pack_graph(val(bits), deg, nbr), codes=codes, pivots=pivots,
                             centroid=np.zeros(D, np.float32), chunk_off=np.arange(0, D + 1, 4, dtype=np.uint32))
    return ix, np.ascontiguousarray(val(qbits))


# ---------------------------------------------------------------------------------------------------------------------
# (g) the vector layouts at either end of what the kernels evaluate
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    # N,   D,   dtype,   R,  m,  Q
    (600, 16,  "uint8", 32, 8,  12),      # G = 1: one lane per survivor
    (600, 32,  "int8",  8,  16, 12),      # G = 2, a tiny degree bound
    (600, 32,  "uint8", 64, 8,  12),      # G = 2, full rows
    (600, 256, "int8",  64, 64, 8),       # G = 16: 4 survivors per wave instruction, the largest integer sums
    (600, 256, "uint8", 32, 64, 8),
    (600, 4,   "float", 8,  2,  12),      # a single 16-byte load per vector
    (600, 20,  "float", 32, 10, 12),      # D % 16 != 0: a partial group of loads
    (600, 68,  "float", 64, 17, 12),      # one dword past a 64-element query register
    (600, 132, "float", 32, 33, 12),      # one dword past the second
    (600, 252, "float", 64, 63, 8),       # a partial tail in the fourth
    (600, 256, "float", 8,  64, 8),       # all four query registers full
]


def shape_id(s) -> str:
    return f"N{s[0]}-D{s[1]}-{s[2]}-R{s[3]}-m{s[4]}"


@functools.lru_cache(maxsize=None)
def shape_index(shape):
    N, D, dtype, R, m, Q = shape
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=8, seed=2000 + D + R, device="cpu", pq_iters=2)
    return ix, q


# ---------------------------------------------------------------------------------------------------------------------
# what the tests share
# ---------------------------------------------------------------------------------------------------------------------
def first_k(ref, k: int):
    """The results of a search with a smaller k, from those of a search with k = kmax at the same L: in every mode of the two references k
    only cuts the final list (tests/test_edge_inputs.py pins this).  ref = (ids [Q][kmax], dists [kmax][Q], stats)."""
    ids, d, st = ref
    return np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(d[:k, :]), st


def ties_in_top(d: np.ndarray, k: int) -> np.ndarray:
    """bool [Q]: two equal distances among a query's first k results (d: [rank][Q])."""
    dk = d[:k]
    return (dk[1:] == dk[:-1]).any(axis=0)
