"""Label tables and filter batches of the label-filter tests (tests/test_labels_mode.py, tests/test_gpu_labels.py).  TEST INFRASTRUCTURE ONLY (a helper
module, not a conftest).  Everything is a function of the index and a fixed seed.

Tables (u32 [N]):
    rand4      bits 0 .. 3 set independently with probability 0.5 / 0.25 / 0.1 / 0.03
    edges      bit 31 on the ids {0, 31, 32, N - 1, medoid}: the first and last bit of a bitmap word, the last node, the seed of every walk
    nobody     all zero: a filter that asks for any bit matches no node
    one_node   query i owns bit i, set on ONE node: the rank-0 result of query i's unfiltered search (at most 32 queries)

Batches (any u32 [Q], all u32 [Q]):
    all2       all = bits 0 and 1 (share 1/8)
    any_all    any = bits 1 | 2, all = bit 0
    mixed      every third query unfiltered (any = all = 0), the others any = bit 2 (share 1/10)
    bit31      any = bit 31 -- for the tables edges and nobody
    own_bit    any = bit i for query i -- for the table one_node
"""
from __future__ import annotations

import numpy as np

SEED = 20260
RAND4_P = (0.5, 0.25, 0.1, 0.03)


def rand4(N: int, seed: int = SEED) -> np.ndarray:
    rng = np.random.default_rng(seed)
    lab = np.zeros(N, np.uint32)
    for b, p in enumerate(RAND4_P):
        lab |= (rng.random(N) < p).astype(np.uint32) << np.uint32(b)
    return lab


def edges(ix) -> np.ndarray:
    lab = np.zeros(int(ix.N), np.uint32)
    lab[[0, 31, 32, int(ix.N) - 1, int(ix.medoid)]] = np.uint32(1) << np.uint32(31)
    return lab


def nobody(N: int) -> np.ndarray:
    return np.zeros(N, np.uint32)


def one_node(N: int, rank0) -> np.ndarray:
    """rank0: the rank-0 id of every query's unfiltered search (<= 32 queries, none padded)"""
    rank0 = np.asarray(rank0, np.uint64).reshape(-1)
    assert len(rank0) <= 32 and int(rank0.max()) < N
    lab = np.zeros(N, np.uint32)
    for i, x in enumerate(rank0):
        lab[int(x)] |= np.uint32(1) << np.uint32(i)
    return lab


def batch(name: str, Q: int):
    any_ = np.zeros(Q, np.uint32)
    all_ = np.zeros(Q, np.uint32)
    if name == "all2":
        all_[:] = 0b0011
    elif name == "any_all":
        any_[:] = 0b0110
        all_[:] = 0b0001
    elif name == "mixed":
        any_[:] = 0b0100
        any_[::3] = 0
    elif name == "bit31":
        any_[:] = np.uint32(1) << np.uint32(31)
    elif name == "own_bit":
        assert Q <= 32
        any_[:] = np.uint32(1) << np.arange(Q, dtype=np.uint32)
    elif name != "none":
        raise ValueError(name)
    return any_, all_


CASES = (("rand4", "all2"), ("rand4", "any_all"), ("rand4", "mixed"), ("edges", "bit31"), ("nobody", "bit31"), ("one_node", "own_bit"))


def table(name: str, ix, rank0=None) -> np.ndarray:
    if name == "rand4":
        return rand4(int(ix.N))
    if name == "edges":
        return edges(ix)
    if name == "nobody":
        return nobody(int(ix.N))
    if name == "one_node":
        return one_node(int(ix.N), rank0)
    raise ValueError(name)
