"""CPU reference of inserts (bang_insert_e; DESIGN.md section 2 CANON 21, section 4.15), composed from ``exact_reference.Reference``.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``insert(ix, vectors, L_build, alpha) -> (Index', stats)`` restates the six steps in
numpy:

1. candidates of a new vector = the final worklist of ``search_one(v, k = L, L, mode="exact")`` on the index AS IT WAS, pad entries dropped;
2. ``prune``: RobustPrune on squared distances -- walk j ascending; an alive c_j joins the row (stop at R ids), else every alive c_t behind it
   dies if ``alpha2 * exact(vector(c_t), query = vector(c_j)) <= d_t`` in float32, ``alpha2 = fl32(fl32(alpha) * fl32(alpha))``; an entry that is
   the list's own node is dropped first;
3. the new entries ``[vector][u32 degree][u32 id x R]``, unused slots 0 (``formats.pack_graph``);
4. back-edges: old node t with the new ids I_t (ascending) that list it -- appended while ``deg_t + |I_t| <= R``, else candidates = old row ++
   I_t cut at 512, distances ``exact(vector(c), query = vector(t))``, sorted by the key (distance bits << 32) | id with equal keys once, pruned;
5. ``code[c]`` = the lowest k minimising ``orc_lut_build``'s table entry ``lut[c][k]`` with the new vector as the query;
6. N grows by n; the medoid stays.

stats: dict(inserted, appended, pruned, dropped, medoid_row_changed, max_incoming, targets, target_pruned) -- ``targets`` are the old nodes the
new rows list, ascending (the order of bang_insert_group's CSR, so a chunk of the back-edge step is a slice of it), ``target_pruned[i]`` says
whether targets[i] overflowed (pruned) or took its ids by appending.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from bang_amd import formats
from bang_amd.binding import NP_DTYPE
from exact_reference import Reference

PRUNE_MAX = 512
PAD = np.uint64(np.iinfo(np.uint64).max)


def alpha2_of(alpha: float) -> np.float32:
    a = np.float32(alpha)
    return np.float32(a * a)


def vector_of(ref: Reference, node: int) -> np.ndarray:
    ix = ref.ix
    vb = ix.D * ref.tsize
    return np.ascontiguousarray(ref.graph[node, :vb]).view(NP_DTYPE[ix.dtype]).copy()


def prune(ref: Reference, own: int, ids, dists, R: int, alpha2, strict: bool = False, wide: bool = False, ties: list | None = None) -> np.ndarray:
    """RobustPrune of the ordered list (ids[j], dists[j]) -> the row's ids (uint32, at most R).

    The rule is the default.  Two WRONG variants exist so that tests/test_insert_reference.py can show that an input tells them apart:
    ``strict`` kills on ``<`` instead of ``<=``; ``wide`` forms ``alpha2 * e`` in float64 instead of rounding the product to float32.
    ``ties`` (a list) receives, per picked candidate, the number of kills decided at ``alpha2 * e == d_t`` exactly."""
    ids = np.asarray(ids, dtype=np.uint32)
    dists = np.asarray(dists, dtype=np.float32)
    keep = ids != np.uint32(own)
    ids, dists = ids[keep], dists[keep]
    alpha2 = np.float32(alpha2)
    alive = np.ones(len(ids), dtype=bool)
    out = []
    for j in range(len(ids)):
        if not alive[j]:
            continue
        out.append(ids[j])
        if len(out) == R:
            break
        t = np.nonzero(alive[j + 1:])[0] + j + 1
        if len(t) == 0:
            break
        e = ref.exact(ids[t], vector_of(ref, int(ids[j])))
        scaled = np.float64(alpha2) * e.astype(np.float64) if wide else (alpha2 * e).astype(np.float32)
        dead = scaled < dists[t] if strict else scaled <= dists[t]
        if ties is not None:
            ties.append(int((dead & (scaled == dists[t])).sum()))
        alive[t[dead]] = False
    return np.array(out, dtype=np.uint32)


def candidates(ref: Reference, v: np.ndarray, L: int):
    """Step 1: the final worklist of the exact walk at k = L, in the order the walk leaves it."""
    ids, dists, _ = ref.search_one(v, L, L, "exact")
    n = int(np.argmax(ids == PAD)) if (ids == PAD).any() else len(ids)
    return ids[:n].astype(np.uint32), dists[:n].copy()


def sort_unique(ids: np.ndarray, dists: np.ndarray):
    """ascending by (distance bits << 32) | id, equal keys once: the key and the result of range_sort_kernel"""
    key = (dists.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
    key = np.unique(key)
    return (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), (key >> np.uint64(32)).astype(np.uint32).view(np.float32)


def encode(ref: Reference, v: np.ndarray) -> np.ndarray:
    return np.argmin(ref.orc.lut_build(v), axis=1).astype(np.uint8)      # (argmin: the first = lowest k of equal entries)


def insert(ix, vectors: np.ndarray, L_build: int, alpha: float):
    vectors = np.ascontiguousarray(vectors, dtype=NP_DTYPE[ix.dtype])
    n, N, R = vectors.shape[0], ix.N, ix.R
    a2 = alpha2_of(alpha)
    old = Reference(ix)
    # steps 1 + 2 + 5 on the index as it was
    lists = [candidates(old, vectors[i], L_build) for i in range(n)]
    rows = [prune(old, N + i, lists[i][0], lists[i][1], R, a2) for i in range(n)]
    codes = np.stack([encode(old, vectors[i]) for i in range(n)])
    # step 3
    deg = np.array([len(r) for r in rows], dtype=np.uint32)
    adj = np.zeros((n, R), dtype=np.uint32)
    for i, r in enumerate(rows):
        adj[i, :len(r)] = r
    graph = np.concatenate([ix.graph, formats.pack_graph(vectors, deg, adj)])
    grown = dataclasses.replace(ix, N=N + n, graph=graph, codes=np.concatenate([ix.codes, codes]))
    ref = Reference(grown)                                               # (vectors of old and new nodes; its graph is the array edited below)
    # step 4
    incoming = {}
    for i, r in enumerate(rows):
        for t in r:
            incoming.setdefault(int(t), []).append(N + i)
    st = dict(inserted=n, appended=0, pruned=0, dropped=0, medoid_row_changed=int(ix.medoid) in incoming,
              max_incoming=max((len(v) for v in incoming.values()), default=0),
              targets=np.array(sorted(incoming), dtype=np.uint32), target_pruned=np.zeros(len(incoming), dtype=bool))
    vb = ix.D * old.tsize
    g = ref.graph
    for ti, t in enumerate(sorted(incoming)):
        assert t < N
        new = np.array(sorted(incoming[t]), dtype=np.uint32)
        row = g[t, vb:].view(np.uint32)                                  # [degree][id x R], a view: edits land in the graph
        d = min(int(row[0]), R)
        if d + len(new) <= R:
            row[1 + d: 1 + d + len(new)] = new
            row[0] = d + len(new)
            st["appended"] += 1
            continue
        cand = np.concatenate([row[1: 1 + d].copy(), new])
        if len(cand) > PRUNE_MAX:
            st["dropped"] += len(cand) - PRUNE_MAX
            cand = cand[:PRUNE_MAX]
        cd = ref.exact(cand, vector_of(ref, t))
        cand, cd = sort_unique(cand, cd)
        out = prune(ref, t, cand, cd, R, a2)
        row[1:] = 0
        row[1: 1 + len(out)] = out
        row[0] = len(out)
        st["pruned"] += 1
        st["target_pruned"][ti] = True
    return dataclasses.replace(grown, graph=g), st
