"""Inputs of the consolidation tests: the delete sets and the crafted graphs.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_consolidate_reference.py asserts ON THE CPU REFERENCE that these inputs
reach their edges; tests/test_gpu_consolidate.py runs them on the GPU.

    ball()             the k nearest points of a node, the node itself among them: a delete set whose members list each other
    CASES, case()      (Index, delete set, alpha) of every engine case; reference() = consolidate_reference.consolidate on it, computed once
    cut index          N = 600, R = 64, D = 16: the 12 nearest points of node 5 gone, lists pass 512 entries
    sparse()           a crafted graph: an affected node whose list ends empty, one whose list is three ids (two equal), a removed row that lists p
    lattice_graph()    insert_inputs' lattice points ("tern6", "plane7") with random rows: lists full of ties for the kill rule
    scan_graph()       N = 130 hand-built rows at R = 5, 16, 64 for the scan / clear kernels
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import insert_inputs as I
from bang_amd import formats, synth
from bang_amd.binding import NP_DTYPE


def ball(ix, node: int, k: int) -> np.ndarray:
    """the k nearest points of `node` (itself first), ascending by squared distance in float64, ties by id"""
    v = ix.vectors().astype(np.float64)
    d = ((v - v[node]) ** 2).sum(axis=1)
    return np.argsort(d, kind="stable")[:k].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def cut_index():
    ix, _, _, _ = synth.make_index(600, 16, "uint8", 64, 8, 4, K=10, n_clusters=8, seed=77, device="cpu", pq_iters=2)
    return ix


def _index(name: str):
    if name == "cut":
        return cut_index()
    if name in I.LAYOUTS:
        return I.layout(name)
    if name.startswith("lattice_"):
        return lattice_graph(name[8:])
    if name == "sparse":
        return sparse()[0]
    return I.get(name)[0]


# name -> (index, how the delete set is made, alpha)
CASES = {
    "i8_ball24":     ("i8", ("ball", 0, 24), 1.2),          # around node 0: one of the balls that reach into the medoid's row
    "i8_ball8_med":  ("i8", ("ball", "medoid", 8), 1.2),    # the medoid is in the set
    "deep_ball4":    ("deep", ("ball", None, 4), 1.2),
    "cut_ball12":    ("cut", ("ball", 5, 12), 1.2),
    "lattice_tern6": ("lattice_tern6", ("random", 20), 1.0),
    "lattice_plane7": ("lattice_plane7", ("random", 20), 1.2),
    "sparse":        ("sparse", ("sparse",), 1.2),
}
CASES.update({"layout_" + k: (k, ("random", 30), 1.2) for k in sorted(I.LAYOUTS)})


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (Index, delete set u32, alpha); read-only"""
    iname, how, alpha = CASES[name]
    ix = _index(iname)
    rng = np.random.default_rng(8800 + sum(map(ord, name)))
    if how[0] == "ball":
        node = int(rng.integers(ix.N)) if how[1] is None else int(ix.medoid) if how[1] == "medoid" else int(how[1])
        x = ball(ix, node, how[2])
    elif how[0] == "random":
        x = np.sort(rng.choice(ix.N, how[1], replace=False)).astype(np.uint32)
    else:
        x = sparse()[1]
    return ix, x, alpha


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """-> (Index', stats, remaining) of consolidate_reference.consolidate on the case; computed once, treat as read-only."""
    import consolidate_reference as CR
    ix, x, alpha = case(name)
    return CR.consolidate(ix, x, alpha)


# ---------------------------------------------------------------------------------------------------------------------
# crafted graphs
# ---------------------------------------------------------------------------------------------------------------------
def with_rows(ix, rows: dict):
    """ix with the rows of the given nodes replaced: {node: ids}"""
    g = ix.graph.copy()
    vb = ix.D * (4 if ix.dtype == "float" else 1)
    for p, ids in rows.items():
        r = g[p, vb:].view(np.uint32)
        r[:] = 0
        r[0] = len(ids)
        r[1: 1 + len(ids)] = ids
    return dataclasses.replace(ix, graph=g)


SPARSE_EMPTY, SPARSE_ONE = 20, 21


@functools.lru_cache(maxsize=None)
def sparse():
    """-> (Index, delete set): the "u8_16" layout index (N = 300, R = 16) with hand-made rows.  D = {10, 11, 12}.  Node 20 lists 10 and 11 only,
    whose rows list removed nodes and 20 itself: its list ends EMPTY.  Node 21 lists 12 and 10: the candidates 30, 30 and 20 -- a list shorter than
    R with a duplicate."""
    ix = I.layout("u8_16")
    assert ix.medoid not in (10, 11, 12, SPARSE_EMPTY, SPARSE_ONE, 30)
    ix = with_rows(ix, {SPARSE_EMPTY: [10, 11], SPARSE_ONE: [12, 10], 10: [11, SPARSE_EMPTY, 12], 11: [SPARSE_EMPTY], 12: [SPARSE_ONE, 30, 10, 30]})
    return ix, np.array([10, 11, 12], np.uint32)


@functools.lru_cache(maxsize=None)
def lattice_graph(kind: str):
    """insert_inputs.lattice("i8", kind) -- 300 lattice points, D = 64, R = 32 -- with a row of 32 random distinct ids (never itself) per node"""
    ix = I.lattice("i8", kind)
    rng = np.random.default_rng(31 + len(kind))
    rows = {}
    for p in range(ix.N):
        ids = rng.choice(ix.N - 1, ix.R, replace=False)
        rows[p] = (ids + (ids >= p)).astype(np.uint32)
    return with_rows(ix, rows)


SCAN_N = 130


@functools.lru_cache(maxsize=None)
def scan_graph(R: int, medoid_excluded: bool = True):
    """-> (graph u8 [130][entry_len], D_vec = 16 uint8, medoid, excluded ids, want affected ids, bad node, bad id).  N = 130 crosses the bitmap word
    and the 64-node seams.  Removed: 3, 31, 32, 64, 129; the medoid 65 is excluded too and counts as live.
      node 0    degree 0                                 node 1    degree R, lists no removed id
      node 2    removed id in the FIRST slot             node 4    removed id in the LAST slot (slot R - 1)
      node 5    degree word R + 9 over a row whose last slot is removed (read as R)
      node 6    a removed id BEHIND its degree (slot 1 at degree 1): not affected
      node 3    removed, lists removed 31 and live 7: not flagged        node 65   the excluded medoid, lists 64: flagged as live
      node 66   lists the medoid only: not affected      node 128  lists 129 (the last node, bit 1 of word 4)
      node 127  slot 0 live, slot 1 an id >= N (never dereferenced, abort = 2), slot 2 removed -- behind the bad id: not affected
    """
    N = SCAN_N
    rng = np.random.default_rng(R)
    vec = rng.integers(0, 255, (N, 16)).astype(np.uint8)
    gone = [3, 31, 32, 64, 129]
    med = 65
    live = [x for x in range(N) if x not in gone]
    deg = np.zeros(N, np.uint32)
    adj = np.zeros((N, R), np.uint32)
    for p in range(N):                                                   # sound rows of live ids first
        k = int(rng.integers(1, R + 1))
        deg[p] = k
        adj[p, :k] = rng.choice([x for x in live if x != p and x != med], k, replace=False) if k <= len(live) - 2 else 0
    deg[0], adj[0] = 0, 0
    deg[1] = R
    adj[1] = rng.choice([x for x in live if x not in (1, med)], R, replace=False)
    adj[2, 0] = 31
    deg[4] = R
    adj[4] = rng.choice([x for x in live if x not in (4, med)], R, replace=False)
    adj[4, R - 1] = 129
    deg[5] = R + 9
    adj[5] = rng.choice([x for x in live if x not in (5, med)], R, replace=False)
    adj[5, R - 1] = 32
    deg[6] = 1
    adj[6, :] = 0
    adj[6, 0], adj[6, 1] = 7, 64
    deg[3] = 2
    adj[3, :] = 0
    adj[3, :2] = [31, 7]
    deg[med] = 2
    adj[med, :] = 0
    adj[med, :2] = [64, 8]
    deg[66] = 1
    adj[66, :] = 0
    adj[66, 0] = med
    deg[128] = 1
    adj[128, :] = 0
    adj[128, 0] = 129
    bad_id = N + 5
    deg[127] = 3
    adj[127, :] = 0
    adj[127, :3] = [9, bad_id, 3]
    graph = formats.pack_graph(vec, deg, adj)
    excluded = np.array(gone + ([med] if medoid_excluded else []), np.uint32)
    want = np.array([2, 4, 5, med, 128], np.uint32)
    return graph, med, excluded, want, 127, bad_id


def bitmap_of(ids, n_nodes: int) -> np.ndarray:
    """the exclusion bitmap as the engine lays it out: ceil(n_nodes / 32) words + one of slack"""
    bits = np.zeros((n_nodes + 31) // 32 + 1, np.uint32)
    for x in np.asarray(ids, np.int64):
        bits[x >> 5] |= np.uint32(1 << (x & 31))
    return bits
