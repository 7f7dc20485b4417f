"""CPU reference of the exact scan (CANON 23).  TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

The distance of EVERY node to every query by ``orc_exact_dist`` through ctypes (as ``exact_reference.Reference.exact`` calls it), the candidate
masks in numpy -- excluded, removed, label filter by CANON 18's rule --, and ``np.sort`` of the 64-bit keys (distance bits << 32) | id.  For 8-bit
data ``distances_int`` is a second path in plain int64 numpy that does not touch the oracle.

    distances(ix, q)           float32 [Q][N], cached per (index object, queries object): compute once, share, leave unchanged
    distances_int(ix, q)       the same for 8-bit vectors from int64 arithmetic
    answer(dist, k, ...)       -> ids u64 [Q][k], dists f32 [k][Q], matched u32 [Q]; padded with UINT64_MAX / 3.402823E+38
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as O

PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
BIG_DIST = np.float32(3.402823e38)

_cache = {}


def distances(ix, q: np.ndarray) -> np.ndarray:
    """float32 [Q][N]: orc_exact_dist(vector(x), raw query), x over all N nodes (whatever their state: the masks come later)."""
    key = (id(ix), id(q))
    hit = _cache.get(key)
    if hit is not None and hit[0] is ix and hit[1] is q:
        return hit[2]
    fn = O.lib().orc_exact_dist
    qq = np.ascontiguousarray(q, dtype=O.NP_DTYPE[ix.dtype])
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)
    base, el = graph.ctypes.data, int(ix.entry_len)
    D, code, zero = C.c_uint32(ix.D), C.c_int(O.DTYPE_CODE[ix.dtype]), C.c_int(0)
    out = np.empty((qq.shape[0], int(ix.N)), np.float32)
    for i in range(qq.shape[0]):
        qp = C.c_void_p(qq[i].ctypes.data)
        row = out[i]
        for x in range(int(ix.N)):
            row[x] = fn(C.c_void_p(base + x * el), qp, D, code, zero)
    out.setflags(write=False)
    _cache[key] = (ix, q, out)
    return out


def distances_int(ix, q: np.ndarray) -> np.ndarray:
    """The 8-bit distances as exact integers (int64 numpy), as float32: every sum is below 2^24."""
    assert ix.dtype in ("uint8", "int8")
    v = ix.vectors().astype(np.int64)
    qq = np.asarray(q).astype(np.int64)
    out = np.empty((qq.shape[0], v.shape[0]), np.int64)
    for i in range(qq.shape[0]):
        d = v - qq[i][None, :]
        out[i] = (d * d).sum(axis=1)
    assert int(out.max(initial=0)) < (1 << 24)
    return out.astype(np.float32)


def bitmap_mask(ids, N: int) -> np.ndarray:
    m = np.zeros(N, bool)
    ids = np.asarray(ids, np.int64).reshape(-1)
    m[ids] = True
    return m


def candidates(N: int, Q: int, excluded=None, removed=None, labels=None, any_=None, all_=None) -> np.ndarray:
    """bool [Q][N]: CANON 23's candidate sets"""
    live = np.ones(N, bool)
    if excluded is not None:
        live &= ~bitmap_mask(excluded, N)
    if removed is not None:
        live &= ~bitmap_mask(removed, N)
    cand = np.broadcast_to(live, (Q, N)).copy()
    if any_ is not None:
        lab = np.asarray(labels, np.uint32)[None, :]
        a = np.asarray(any_, np.uint32)[:, None]
        b = np.asarray(all_, np.uint32)[:, None]
        cand &= ((a == 0) | ((lab & a) != 0)) & ((lab & b) == b)
    return cand


def answer(dist: np.ndarray, k: int, excluded=None, removed=None, labels=None, any_=None, all_=None, n_nodes=None):
    """dist: float32 [Q][N] (distances / distances_int); n_nodes: scan the prefix [0, n_nodes) only."""
    Q, N = dist.shape
    n = N if n_nodes is None else int(n_nodes)
    cand = candidates(N, Q, excluded, removed, labels, any_, all_)[:, :n]
    bits = np.ascontiguousarray(dist[:, :n]).view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    ids = np.full((Q, k), PAD_ID, np.uint64)
    dists = np.full((k, Q), BIG_DIST, np.float32)
    matched = cand.sum(axis=1).astype(np.uint32)
    for i in range(Q):
        s = np.sort(keys[i][cand[i]])[:k]
        ids[i, :len(s)] = s & np.uint64(0xFFFFFFFF)
        dists[:len(s), i] = (s >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return ids, dists, matched


def same(got, want) -> bool:
    """ids, distance bits and matched, bit for bit"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1]).view(np.uint32), np.asarray(want[1]).view(np.uint32))
            and np.array_equal(got[2], want[2]))


def first_difference(got, want) -> str:
    for name, a, b in (("ids", got[0], want[0]), ("dists", np.asarray(got[1]).view(np.uint32).T, np.asarray(want[1]).view(np.uint32).T),
                       ("matched", got[2], want[2])):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return f"{name}: shape {a.shape} vs {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            at = tuple(int(x) for x in bad[0])
            return f"{name}: {len(bad)} differ, first at query/rank {at}: got {a[at]!r}, want {b[at]!r}"
    return "equal"
