"""Inputs and references for option vectors_fp16 (the HBM vector table of a float index held as IEEE fp16).

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  fp16 -> fp32 is exact, so what the engine must return with the option on is what
the CPU references (oracle.Oracle.search; tests/exact_reference.py in exact mode) return on a COPY of the index whose graph-entry vectors are
v.astype(float16).astype(float32) -- PQ codes, pivots, adjacency and queries as they are.  tests/test_fp16_inputs.py asserts on the CPU that on
every input used by tests/test_gpu_vectors_fp16.py that reference differs from the one on the original index, so the GPU comparison cannot pass
by ignoring the option.

    rounded()           the copy
    row_bytes(), table_bytes()   the table's geometry (bang_stats.vector_table_bytes)
    synth_index()       synth.make_index at D = 7, 33, 100, 260 (re-rank) and D = 256 (exact mode)
    rounding_ties()     edge_inputs.tie_heavy on a float fixture plus pairs of nodes that differ only below fp16 precision
    off_grid()          a float toy of edge_inputs (integer vectors, exact in fp16) moved off the fp16 grid: its rounded copy IS the toy
    pq_reference(), exact_reference()   the references, computed once per (input, k, L)
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from bang_amd import synth
from bang_amd.formats import pack_graph

# D -> (N, R, m, Q).  7: an odd row (a padding half); 33: odd and a partial dword tile; 100: D % 8 != 0; 260: beyond 256 -- a second tile of the
# re-rank's fetch, and a layout on the LUT path (no search-kernel instance: the host placement runs the launch-per-iteration loop)
SYNTH = {7: (800, 16, 7, 24), 33: (1200, 32, 11, 24), 100: (1500, 64, 25, 32), 260: (900, 32, 65, 16), 256: (1200, 64, 64, 24)}


def row_bytes(D: int) -> int:
    return (2 * D + 3) & ~3


def table_bytes(N: int, D: int) -> int:
    return N * row_bytes(D) + 256


def rounded(ix):
    """The index the engine effectively searches with vectors_fp16 = 1."""
    assert ix.dtype == "float"
    v = ix.vectors().astype(np.float16).astype(np.float32)
    return dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency()))


@functools.lru_cache(maxsize=None)
def synth_index(D: int):
    N, R, m, Q = SYNTH[D]
    ix, q, _, _ = synth.make_index(N, D, "float", R, m, Q, K=10, n_clusters=8, seed=4000 + D, device="cpu", pq_iters=2)
    return ix, q


def rounding_ties(ix, q):
    """edge_inputs.tie_heavy (small integers: exact in fp16, ties everywhere) with every odd node 2j + 1 a copy of node 2j whose non-zero
    coordinates are scaled by 1 + 2^-14 -- far below half an fp16 ulp, so the pair differs in fp32 and is ONE vector after rounding: exact
    ties between different nodes that only the rounded table has, broken by expansion order."""
    import edge_inputs as E
    ix2, q2 = E.tie_heavy(ix, q)
    v = ix2.vectors()
    n = (ix2.N // 2) * 2
    v[1:n:2] = v[0:n:2] * np.float32(1.0 + 2.0 ** -14)
    assert not np.array_equal(v[1:n:2], v[0:n:2])
    out = dataclasses.replace(ix2, graph=pack_graph(v, ix2.degrees(), ix2.adjacency()))
    r = rounded(out).vectors()
    assert np.array_equal(r[1:n:2], r[0:n:2])
    return out, q2


def off_grid(ix):
    """A float toy of edge_inputs holds integer levels (0 .. 255, exact in fp16): every vector scaled by 1 + 2^-12, at most half an fp16 ulp,
    rounds back to the toy -- so the rounded reference walks the toy (its ties, its 65-id seed list, its chain to the cap) while the original
    index has other distance bits."""
    v = ix.vectors() * np.float32(1.0 + 2.0 ** -12)
    out = dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency()))
    assert np.array_equal(rounded(out).vectors(), ix.vectors())
    return out


_REF = {}


def pq_reference(key, ix, q, k, L, mips=False):
    """Oracle.search on ix AS GIVEN (pass rounded(ix) for the fp16 expectation): (ids, dists, stats)."""
    from oracle import oracle as O
    if ("pq", key, k, L, mips) not in _REF:
        _REF[("pq", key, k, L, mips)] = O.Oracle(ix).search(q, k, L, mips=mips, with_stats=True)
    return _REF[("pq", key, k, L, mips)]


def exact_reference(key, ix, q, k, L):
    from exact_reference import Reference
    if ("exact", key, k, L) not in _REF:
        _REF[("exact", key, k, L)] = Reference(ix).search(q, k, L, "exact")
    return _REF[("exact", key, k, L)]


def distance_bits_differ(a, b) -> bool:
    return not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
