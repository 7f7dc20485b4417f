"""Inputs of the exact-scan tests (tests/test_scan_reference.py on the CPU, tests/test_gpu_scan.py on the GPU).  TEST INFRASTRUCTURE ONLY (a helper
module, not a conftest).  Everything is a function of a fixed seed; treat every returned array as read-only.

    FIXTURES            the session fixtures of conftest.py the tests scan: small_u8 (N = 4000, D = 128), small_i8 (2000, 64), small_f32 (3000, 128),
                        small_deep (2500, 96: not a multiple of 32)
    SMALL, small()      8-bit indexes of N = 640 at D = 16 (half a k-step of the MFMA), 32 (one) and 256 (eight), made as stretch_inputs.get makes its own
    extremes()          rows of all 0 / all 255 (u8), all -128 / all 127 (i8) at D = 256, each queried with the opposite row: the largest sum
                        256 x 255^2 = 16 646 400, the ^ 0x80 shift, the sign handling
    ties()              N = 200, 50 copies of one vector on ids that straddle the 32-point tiles and the ends of stripes; the query is close to the
                        copies, so rank k falls inside the tie group for every k the tests use below 50 and the lowest ids must win
    label cases         labels_inputs.CASES: (table, batch) names; `nobody` leaves no candidate, `mixed` holds unfiltered queries
    exclusion sets      excl_ranks(): each query's true ranks 0 .. 4; excl_all_but(): all nodes but three; excl_edges(): the bitmap-word edges
    KS                  the k every input is scanned at
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import labels_inputs as LI
from bang_amd import synth

FIXTURES = ("small_u8", "small_i8", "small_f32", "small_deep")
KS = (1, 10, 100, 128)
QS = (1, 31, 33, 130)
N_PREFIXES = (1, 31, 32, 33, 63, 64, 65)          # and N itself
LABEL_CASES = LI.CASES

# name -> (D, dtype, m)
SMALL = {"u8_16": (16, "uint8", 8), "i8_16": (16, "int8", 8), "u8_32": (32, "uint8", 8), "i8_32": (32, "int8", 8), "u8_256": (256, "uint8", 32),
         "i8_256": (256, "int8", 32)}
SMALL_N, SMALL_R, SMALL_Q = 640, 32, 16


@functools.lru_cache(maxsize=None)
def small(name: str):
    """-> (Index, queries [16][D])"""
    D, dtype, m = SMALL[name]
    ix, q, _, _ = synth.make_index(SMALL_N, D, dtype, SMALL_R, m, SMALL_Q, K=10, n_clusters=8, seed=7000 + D + m + (dtype == "int8"), device="cpu", pq_iters=2)
    return ix, np.ascontiguousarray(q)


def with_vectors(ix, vectors: np.ndarray):
    """ix cut to its first len(vectors) nodes with their vectors replaced; the rows become a ring (node i lists i + 1 .. i + R mod n: a scan never
    reads them, a load checks them)"""
    from bang_amd import formats
    n = vectors.shape[0]
    deg = min(int(ix.R), n - 1)
    adj = np.zeros((n, int(ix.R)), np.uint32)
    adj[:, :deg] = (np.arange(n, dtype=np.uint32)[:, None] + 1 + np.arange(deg, dtype=np.uint32)[None, :]) % np.uint32(n)
    g = formats.pack_graph(np.ascontiguousarray(vectors), np.full(n, deg, np.uint32), adj)
    assert g.shape == (n, ix.entry_len)
    return dataclasses.replace(ix, N=n, graph=g, codes=ix.codes[:n].copy(), medoid=0)


EXTREME_MAX = 256 * 255 * 255


@functools.lru_cache(maxsize=None)
def extremes(dtype: str):
    """-> (Index of N = 64 at D = 256, queries [2][256]): rows alternate lowest / highest value; query 0 is all lowest, query 1 all highest"""
    ix0, _ = small("u8_256" if dtype == "uint8" else "i8_256")
    lo, hi = (0, 255) if dtype == "uint8" else (-128, 127)
    npdt = np.uint8 if dtype == "uint8" else np.int8
    v = np.empty((64, 256), npdt)
    v[0::2] = lo
    v[1::2] = hi
    q = np.stack([np.full(256, lo, npdt), np.full(256, hi, npdt)])
    return with_vectors(ix0, v), q


TIE_N = 200
TIE_IDS = tuple([0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 95, 96, 97, 126, 127, 128, 129, 130, 158, 159, 160, 161, 190, 191, 192, 193, 198, 199]
                + list(range(100, 122)))


@functools.lru_cache(maxsize=None)
def ties(kind: str):
    """kind: "u8" (D = 128) or "f32" (D = 128).  -> (Index of N = 200, queries [3][D], the 50 tied ids ascending).  The 50 copies are the nearest
    points of every query by a wide margin; the other points are all different."""
    assert len(set(TIE_IDS)) == 50 and max(TIE_IDS) < TIE_N
    rng = np.random.default_rng(4242)
    if kind == "u8":
        ix0, _ = _fixture_like("uint8")
        v = rng.integers(0, 256, (TIE_N, 128)).astype(np.uint8)
        base = np.full(128, 100, np.uint8)
        q = np.stack([base, base + 1, np.concatenate([base[:64], base[64:] + 2])]).astype(np.uint8)
    else:
        ix0, _ = _fixture_like("float")
        v = (rng.standard_normal((TIE_N, 128)) * 50.0).astype(np.float32)
        base = np.full(128, 0.25, np.float32)
        q = np.stack([base, base + np.float32(0.5), base * np.float32(-1.0)]).astype(np.float32)
    v[list(TIE_IDS)] = base
    return with_vectors(ix0, v), np.ascontiguousarray(q), np.array(sorted(TIE_IDS), np.uint64)


@functools.lru_cache(maxsize=None)
def _fixture_like(dtype: str):
    ix, q, _, _ = synth.make_index(TIE_N, 128, dtype, 32, 32, 4, K=10, n_clusters=4, seed=8100, device="cpu", pq_iters=2)
    return ix, q


def queries_of(q: np.ndarray, Q: int) -> np.ndarray:
    """Q queries from the fixture's: repeated in order (the reference distances of query i are those of query i mod len(q))"""
    return np.ascontiguousarray(q[np.arange(Q) % q.shape[0]])


def tile_dist(dist: np.ndarray, Q: int) -> np.ndarray:
    return dist[np.arange(Q) % dist.shape[0]]


# ------------------------------------------------------------------------------------------------------------------------ exclusion sets
def excl_ranks(dist: np.ndarray) -> np.ndarray:
    """the ids of every query's true ranks 0 .. 4 (dist: the reference distances [Q][N])"""
    N = dist.shape[1]
    keys = (np.ascontiguousarray(dist).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    top = np.sort(keys, axis=1)[:, :5] & np.uint64(0xFFFFFFFF)
    return np.unique(top.astype(np.uint32))


def excl_all_but(N: int) -> np.ndarray:
    keep = {5 % N, N // 2, N - 1}
    return np.array([x for x in range(N) if x not in keep], np.uint32)


def excl_edges(N: int) -> np.ndarray:
    return np.array([0, 31, 32, N - 1], np.uint32)


EXCLUSIONS = ("ranks", "all_but", "edges")


def exclusion(name: str, dist: np.ndarray) -> np.ndarray:
    N = dist.shape[1]
    return {"ranks": lambda: excl_ranks(dist), "all_but": lambda: excl_all_but(N), "edges": lambda: excl_edges(N)}[name]()


def label_case(table: str, batch: str, ix, Q: int, dist: np.ndarray):
    """-> (labels u32 [N], any u32 [Q], all u32 [Q]); one_node needs the unfiltered rank 0 of <= 32 queries: the batch is cut to 32 by the caller"""
    rank0 = None
    if table == "one_node":
        rank0 = np.argmin(dist[:Q], axis=1)          # (the unfiltered nearest; ties to the lowest id, as the scan)
    lab = LI.table(table, ix, rank0)
    a, b = LI.batch(batch, Q)
    return lab, a, b
