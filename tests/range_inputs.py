"""Radii of the range-search tests (tests/test_range_mode.py, tests/test_gpu_range.py).  TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).
Everything is a function of the index and its queries.

Radii (f32 [Q], squared L2 -- the unit the engine returns):
    rank5 / rank100 / rank400   the brute-force distance of each query's rank-N point (the N-th nearest of all N points, by the oracle's exact
                                distance): the point itself is at distance == radius, so the compare's "<=" is on the edge for every query
    none                        -1 for every query: nothing is within a negative radius
    all                         +inf: every evaluated node
    mixed                       rank100, but every third query -1 and query 1 NaN
"""
from __future__ import annotations

import numpy as np

RANKS = (5, 100, 400)
NAMES = ("rank5", "rank100", "rank400", "none", "all", "mixed")
_CACHE = {}


def brute_force(ref, ix, q) -> np.ndarray:
    """f32 [Q][N], every row sorted ascending: orc_exact_dist of every point against every query (ref: an exact_reference.Reference of ix)"""
    key = (id(ix), q.shape, q.tobytes()[:64])
    if key not in _CACHE:
        every = np.arange(int(ix.N), dtype=np.uint32)
        _CACHE[key] = np.stack([np.sort(ref.exact(every, np.ascontiguousarray(q[i]))) for i in range(q.shape[0])])
    return _CACHE[key]


def radii(name: str, ref, ix, q) -> np.ndarray:
    Q = q.shape[0]
    if name == "none":
        return np.full(Q, -1.0, np.float32)
    if name == "all":
        return np.full(Q, np.inf, np.float32)
    if name == "mixed":
        r = brute_force(ref, ix, q)[:, 100 - 1].copy()
        r[::3] = -1.0
        r[1] = np.nan
        return r.astype(np.float32)
    if name.startswith("rank") and int(name[4:]) in RANKS:
        return brute_force(ref, ix, q)[:, int(name[4:]) - 1].astype(np.float32)
    raise ValueError(name)
