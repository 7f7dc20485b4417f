"""CPU reference of inserts that re-use the ids of removed nodes (bang_insert_reuse_e; DESIGN.md section 2 CANON 24, section 4.18), composed from
``insert_reference`` (candidates, prune, encode, sort_unique, vector_of) and ``consolidate_reference``: no new arithmetic.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

    eligible(removed, excluded)     E = F \\ X, ascending
    assign(free, n, N)              f = min(n, |E|); ids[i] = the i-th smallest of E for i < f, N + (i - f) behind
    insert_at(ix, vectors, ids, L_build, alpha) -> (Index', stats)
                                    insert_reference.insert with "N + i" read as ids[i]: the searches and the prune of the new rows run on the index as
                                    it was, entries and codes are written at ids (appended for ids >= N), an old node t takes I_t = sorted(incoming[t])
    insert_reuse(ix, removed, excluded, vectors, L_build, alpha) -> (Index', ids, removed', stats)

With ``removed`` empty this is insert_reference.insert byte for byte (tests/test_reuse_reference.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

import insert_reference as IR
from bang_amd import formats
from bang_amd.binding import NP_DTYPE
from exact_reference import Reference

PRUNE_MAX = IR.PRUNE_MAX


def eligible(removed, excluded) -> np.ndarray:
    return np.setdiff1d(np.asarray(removed, np.int64), np.asarray(excluded, np.int64)).astype(np.uint32)


def assign(free, n: int, N: int) -> np.ndarray:
    free = np.asarray(free, np.uint32)
    f = min(n, len(free))
    return np.concatenate([free[:f], N + np.arange(n - f, dtype=np.uint32)]).astype(np.uint32)


def insert_at(ix, vectors: np.ndarray, ids, L_build: int, alpha: float):
    vectors = np.ascontiguousarray(vectors, dtype=NP_DTYPE[ix.dtype])
    ids = np.asarray(ids, np.uint32)
    n, N, R = vectors.shape[0], ix.N, ix.R
    assert len(ids) == n and (np.diff(ids.astype(np.int64)) > 0).all(), "ids strictly ascending"
    n_app = int((ids >= N).sum())
    assert np.array_equal(ids[n - n_app:], N + np.arange(n_app, dtype=np.uint32)), "the appended ids follow N"
    a2 = IR.alpha2_of(alpha)
    old = Reference(ix)
    # steps 1 + 2 + 5 on the index as it was
    lists = [IR.candidates(old, vectors[i], L_build) for i in range(n)]
    rows = [IR.prune(old, int(ids[i]), lists[i][0], lists[i][1], R, a2) for i in range(n)]
    codes = np.stack([IR.encode(old, vectors[i]) for i in range(n)])
    # step 3: the entries at their slots
    deg = np.array([len(r) for r in rows], dtype=np.uint32)
    adj = np.zeros((n, R), dtype=np.uint32)
    for i, r in enumerate(rows):
        adj[i, :len(r)] = r
    graph = np.concatenate([ix.graph, np.zeros((n_app, ix.graph.shape[1]), np.uint8)])
    graph[ids] = formats.pack_graph(vectors, deg, adj)
    all_codes = np.concatenate([ix.codes, np.zeros((n_app, ix.m), np.uint8)])
    all_codes[ids] = codes
    grown = dataclasses.replace(ix, N=N + n_app, graph=graph, codes=all_codes)
    ref = Reference(grown)
    # step 4
    batch = set(int(x) for x in ids)
    incoming = {}
    for i, r in enumerate(rows):
        for t in r:
            incoming.setdefault(int(t), []).append(int(ids[i]))
    st = dict(inserted=n, appended=0, pruned=0, dropped=0, medoid_row_changed=int(ix.medoid) in incoming,
              max_incoming=max((len(v) for v in incoming.values()), default=0),
              targets=np.array(sorted(incoming), dtype=np.uint32), target_pruned=np.zeros(len(incoming), dtype=bool))
    vb = ix.D * old.tsize
    g = ref.graph
    for ti, t in enumerate(sorted(incoming)):
        assert t < N and t not in batch, "a new row lists a slot of the batch: a free slot was reachable"
        new = np.array(sorted(incoming[t]), dtype=np.uint32)
        row = g[t, vb:].view(np.uint32)
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
        cd = ref.exact(cand, IR.vector_of(ref, t))
        cand, cd = IR.sort_unique(cand, cd)
        out = IR.prune(ref, t, cand, cd, R, a2)
        row[1:] = 0
        row[1: 1 + len(out)] = out
        row[0] = len(out)
        st["pruned"] += 1
        st["target_pruned"][ti] = True
    return dataclasses.replace(grown, graph=g), st


def insert_reuse(ix, removed, excluded, vectors: np.ndarray, L_build: int, alpha: float):
    removed = np.unique(np.asarray(removed, np.uint32))
    free = eligible(removed, excluded)
    n = len(vectors)
    ids = assign(free, n, ix.N)
    f = min(n, len(free))
    ix2, st = insert_at(ix, vectors, ids, L_build, alpha)
    st["reused"] = f
    return ix2, ids, np.setdiff1d(removed, ids[:f]).astype(np.uint32), st
