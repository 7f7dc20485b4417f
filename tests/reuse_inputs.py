"""Inputs of the tests of inserts that re-use the ids of removed nodes, built from ``insert_inputs`` and ``consolidate_inputs``.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_reuse_reference.py asserts ON THE CPU REFERENCE that these inputs reach the
edges they are named for; tests/test_gpu_reuse.py runs them on the GPU.

    case            construction                                                              edge
    mixed           index "i8" consolidated with "i8_ball24", then a 48-point batch           0 < f < n
    all_free        "layout_i8_32" (30 random deletes), a batch of 16 and a second of 16     first batch f == n, second 0 < f < n
    med             "i8_ball8_med"                                                            the medoid stays excluded and is never handed out
    excluded_again  "i8_ball24", then X = {3 of the free ids, 1 live id}                      those three are skipped and stay free
    deep            "deep_ball4" plus 16 points                                               float vectors, m = 74
    u8              index "u8" with 40 random deletes plus 64 points                          m = 70 packed code rows, R = 64
    exact_fit       "i8_ball24", capacity == N, n == |E|                                      a batch bang_insert_e must refuse succeeds

reference(name) -> Run: the consolidated index, F and X in front of the first batch, and per batch (vectors, ids, Index', F', stats)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import consolidate_inputs as CI
import consolidate_reference as CR
import insert_inputs as I

# name -> (consolidation case or None, batches ((n or None = |E|, seed), ...), L_build, alpha, ids excluded again?, capacity == N?)
CASES = {
    "mixed":          ("i8_ball24", ((48, 21),), 40, 1.2, False, False),
    "all_free":       ("layout_i8_32", ((16, 22), (16, 23)), 24, 1.2, False, False),
    "med":            ("i8_ball8_med", ((16, 24),), 40, 1.2, False, False),
    "excluded_again": ("i8_ball24", ((32, 25),), 40, 1.2, True, False),
    "deep":           ("deep_ball4", ((16, 26),), 48, 1.2, False, False),
    "u8":             (None, ((64, 27),), 64, 1.2, False, False),
    "exact_fit":      ("i8_ball24", ((None, 28),), 40, 1.2, False, True),
}
U8_DELETES = 40


@dataclasses.dataclass
class Step:
    vectors: np.ndarray
    ids: np.ndarray            # uint32 [n], the ids of the batch
    ix: object                 # Index' behind the batch
    removed: np.ndarray        # F behind the batch
    stats: dict


@dataclasses.dataclass
class Run:
    ix0: object                # the index as loaded
    x: np.ndarray              # the delete set the engine consolidates
    alpha_c: float
    ix1: object                # ... and the consolidated index
    cons_stats: dict
    excluded: np.ndarray       # X in front of the first batch (what stays of x, and the ids excluded again)
    removed: np.ndarray        # F in front of the first batch
    L: int
    alpha: float
    capacity: int
    steps: list


@functools.lru_cache(maxsize=None)
def consolidated(name: str):
    """-> (Index, delete set, alpha, Index', stats, remaining) of the case's consolidation"""
    cons = CASES[name][0]
    if cons is not None:
        return CI.case(cons) + CI.reference(cons)
    ix, _ = I.get("u8")
    x = np.sort(np.random.default_rng(5150).choice(ix.N, U8_DELETES, replace=False)).astype(np.uint32)
    return (ix, x, 1.2) + CR.consolidate(ix, x, 1.2)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Run:
    """computed once, treat as read-only"""
    import reuse_reference as RR
    _, batches, L, alpha, again, exact = CASES[name]
    ix0, x, alpha_c, ix1, cst, remaining = consolidated(name)
    in_d, _ = CR.split(ix0, x)
    removed = np.flatnonzero(in_d).astype(np.uint32)
    excluded = np.asarray(remaining, np.uint32)
    if again:
        live = int(np.flatnonzero(~in_d & (np.arange(ix0.N) != ix0.medoid))[7])
        excluded = np.union1d(excluded, np.array([removed[1], removed[5], removed[10], live], np.uint32)).astype(np.uint32)
    run = Run(ix0, x, alpha_c, ix1, cst, excluded, removed, L, alpha, 0, [])
    ix, appended = ix1, 0
    for n, seed in batches:
        n = len(RR.eligible(removed, excluded)) if n is None else n
        v = I.batch(ix, n, seed)
        ix2, ids, removed2, st = RR.insert_reuse(ix, removed, excluded, v, L, alpha)
        run.steps.append(Step(v, ids, ix2, removed2, st))
        appended += n - st["reused"]
        ix, removed = ix2, removed2
    run.capacity = ix0.N if exact else ix0.N + appended + 8
    assert not exact or appended == 0
    return run
