"""Small deterministic indexes that drive the BEAM form of the exact-distance walk (options distance = 1, beam = W) to its edges.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  Built with edge_inputs.toy: node i's distance to the query is D * levels[i]^2, so a
lower level is a closer node and equal levels are exact ties.  tests/test_beam_mode.py asserts ON THE CPU REFERENCE (tests/beam_reference.py)
that every input reaches the edge it is named for; tests/test_gpu_exact_beam.py compares the kernels with that reference bit for bit.

    shared_child   nodes 1 and 2 both list node 3 and are expanded together at W = 2: the id survives in both rows and is kept once
    row_tie        a survivor of row 1 ties one of row 0: merged later, it stands in front of it
    row_dup        an id twice in one row: both copies stay, both become parents of one iteration, the second copy's row is dropped whole
    ladder         two parallel falling chains: P = 2 every iteration, until the candidate log has room for one parent only
    fan4           four parents of 64 distinct neighbours each: 256 kept survivors in one iteration at W = 4
and the inputs of tests/edge_inputs.py that matter to the new walk: seed65 (a first row of 65 ids), chain (P = 1 up to the iteration cap),
short_worklist (duplicates inside one row stay) and extreme (8-bit distances just below 2^24).
"""
from __future__ import annotations

import edge_inputs as E

LAYOUTS = (("uint8", 128), ("int8", 64), ("float", 128))     # one per vector type (and per kernel instance)


def shared_child(dtype: str = "uint8", D: int = 128):
    """0 -> {1, 2}; 1 -> {3, 4}; 2 -> {3, 5}.  At W = 2 nodes 1 and 2 are expanded together and node 3 survives the filter in both rows."""
    return E.toy({0: [1, 2], 1: [3, 4], 2: [3, 5]}, [100, 20, 30, 10, 15, 12], dtype, D)


def row_tie(dtype: str = "uint8", D: int = 128):
    """0 -> {1, 2}; 1 -> {3}; 2 -> {4}; nodes 3 and 4 tie.  At W = 2 node 3 comes with row 0 and node 4 with row 1."""
    return E.toy({0: [1, 2], 1: [3], 2: [4]}, [100, 20, 30, 10, 10], dtype, D)


def row_dup(dtype: str = "uint8", D: int = 128):
    """0 -> {1}; 1 -> {2, 2, 3}; 2 -> {4, 5}.  Node 2 stands twice in ONE row: both copies pass the filter (the state at entry) and both stay, so
    the worklist holds node 2 twice; at W = 2 both copies become parents of one iteration, and the second copy's whole row is dropped."""
    return E.toy({0: [1], 1: [2, 2, 3], 2: [4, 5]}, [100, 50, 20, 30, 10, 15], dtype, D)


LADDER_L = 10           # cand_stride = 60: before the selection of iteration 30 the log holds 59 entries -- room for one of the two parents
LADDER_NODES = 80


def ladder(dtype: str = "uint8", D: int = 128):
    """0 -> {1, 2}, i -> {i + 2}: two chains (odd and even nodes) with the distance falling along both.  At W = 2 every iteration expands the
    heads of both chains and finds their two successors, closer than everything before."""
    n = LADDER_NODES
    adj = {0: [1, 2]}
    adj.update({i: [i + 2] for i in range(1, n - 2)})
    return E.toy(adj, [255 - i for i in range(n)], dtype, D)


FAN4_PARENTS = (1, 2, 3, 4)


def fan4(dtype: str = "uint8", D: int = 128):
    """0 -> {1, 2, 3, 4}; parent p -> 64 nodes of its own (5 + 64 (p - 1) ...), 256 distinct ids.  Their levels repeat with period 41, so
    every row ties the other rows many times over; four of them lead on to ever closer nodes."""
    adj = {0: list(FAN4_PARENTS)}
    levels = [200, 100, 101, 102, 103]
    for p in FAN4_PARENTS:
        first = 5 + 64 * (p - 1)
        adj[p] = list(range(first, first + 64))
        levels += [50 + ((first + i) * 7) % 41 for i in range(64)]
    tail = len(levels)                                                # 261 .. 268: closer and closer
    for j, src in enumerate((5, 70, 140, 200)):
        adj[src] = [tail + 2 * j, tail + 2 * j + 1]
        levels += [40 - 4 * j, 38 - 4 * j]
    return E.toy(adj, levels, dtype, D)


# name -> (builder(dtype, D), the beams it is run at, the worklist lengths).  `extreme` takes the vector type alone and has no float form.
INPUTS = {
    "shared_child":   (shared_child, (2, 4), (8, 37)),
    "row_tie":        (row_tie, (2, 3), (3, 8)),
    "row_dup":        (row_dup, (2, 4), (8,)),
    "ladder":         (ladder, (2, 3), (LADDER_L, 37)),
    "fan4":           (fan4, (4, 2), (37, 300)),
    "seed65_best":    (lambda dtype, D: E.seed65(dtype, "best", D), (2, 4), (4, 37)),
    "seed65_tie":     (lambda dtype, D: E.seed65(dtype, "tie", D), (2, 4), (4, 37)),
    "seed65_worse":   (lambda dtype, D: E.seed65(dtype, "worse", D), (3,), (4, 37)),
    "chain":          (E.chain, (2, 4), (10, 37)),
    "short_worklist": (E.short_worklist, (2, 4), (16,)),
    "extreme":        (lambda dtype, D: E.extreme(dtype), (2, 4), (37,)),
}


def cases():
    """(name, dtype, D) of every input in every vector type it exists in."""
    out = []
    for name in INPUTS:
        for dtype, D in LAYOUTS:
            if name == "extreme":
                if dtype == "float":
                    continue
                D = 256
            out.append((name, dtype, D))
    return out


def build(name: str, dtype: str, D: int):
    """-> (ix, queries, beams, Ls)"""
    fn, beams, Ls = INPUTS[name]
    ix, q = fn(dtype, D)
    return ix, q, beams, Ls
