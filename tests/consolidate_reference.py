"""CPU reference of consolidation (bang_consolidate_e; DESIGN.md section 2 CANON 22, section 4.16), composed from ``insert_reference`` (prune,
sort_unique, vector_of) and ``exact_reference.Reference``: no new arithmetic.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  ``consolidate(ix, excluded, alpha) -> (Index', stats, remaining)`` restates the
seven steps in numpy.  X = the excluded ids, med = the medoid, D = X \\ {med}; row(p) = the first min(degree word, R) ids of p's row as it stood
at the call:

1. affected: every p not in D whose row(p) lists an id of D;
2. candidates of p: the ids of row(p) not in D, in row order; then for each v of row(p) in D, in row order, the ids of row(v) that are neither in D
   nor p, in row order; duplicates kept; cut at 512, what the cut drops counted;
3. distances ``exact(vector(c), query = vector(p))``;
4. sorted by the key (distance bits << 32) | id with equal keys once;
5. pruned at alpha2 into p's row (unused slots 0, an empty list gives degree 0);
6. the row of every v in D becomes R + 1 zero words;
7. remaining = X & {med}.

stats: dict(rows, removed, dropped, still_excluded, affected) -- ``affected`` ascending, the order of bang_consolidate_group's list (a chunk of the
gather step is a slice of it).  ``lists(ix, excluded)`` hands out step 2 alone, with what the input tests ask about each list.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import insert_reference as IR
from exact_reference import Reference

PRUNE_MAX = IR.PRUNE_MAX


def split(ix, excluded):
    """-> (in_D bool [N], remaining ids): the removed nodes and what stays excluded (the medoid, if it was)"""
    x = np.unique(np.asarray(excluded, dtype=np.int64))
    assert len(x) == 0 or (x.min() >= 0 and x.max() < ix.N)
    in_d = np.zeros(ix.N, dtype=bool)
    in_d[x] = True
    in_d[ix.medoid] = False
    return in_d, x[x == ix.medoid].astype(np.uint32)


def rows_of(ix):
    deg, adj = np.minimum(ix.degrees(), ix.R), ix.adjacency()
    return [adj[p, :deg[p]] for p in range(ix.N)]


@dataclasses.dataclass
class CandList:
    ids: np.ndarray            # the whole list, before the cut at 512
    lists_p: bool              # a removed row lists p (dropped from the list)
    removed_lists_removed: bool
    n_removed: int             # removed neighbours of p


def lists(ix, excluded):
    """step 1 + 2 -> {p: CandList} over the affected nodes, ascending"""
    in_d, _ = split(ix, excluded)
    rows = rows_of(ix)
    out = {}
    for p in range(ix.N):
        row = rows[p]
        if in_d[p] or not in_d[row].any():
            continue
        parts, lists_p, rlr = [row[~in_d[row]]], False, False
        gone = row[in_d[row]]
        for v in gone:
            rv = rows[int(v)]
            lists_p |= bool((rv == p).any())
            rlr |= bool(in_d[rv].any())
            parts.append(rv[(~in_d[rv]) & (rv != p)])
        out[p] = CandList(np.concatenate(parts).astype(np.uint32), lists_p, rlr, len(gone))
    return out


def consolidate(ix, excluded, alpha: float, strict: bool = False, ref: Reference | None = None):
    """-> (Index', stats, remaining).  ``strict``: the WRONG kill rule '<' of insert_reference.prune, for the input tests."""
    ref = ref or Reference(ix)
    R = ix.R
    a2 = IR.alpha2_of(alpha)
    in_d, remaining = split(ix, excluded)
    cl = lists(ix, excluded)
    vb = ix.D * ref.tsize
    g = ix.graph.copy()
    dropped = 0
    for p, c in cl.items():
        cand = c.ids
        if len(cand) > PRUNE_MAX:
            dropped += len(cand) - PRUNE_MAX
            cand = cand[:PRUNE_MAX]
        d = ref.exact(cand, IR.vector_of(ref, p))
        cand, d = IR.sort_unique(cand, d)
        out = IR.prune(ref, p, cand, d, R, a2, strict=strict)
        row = g[p, vb:].view(np.uint32)                                  # [degree][id x R], a view
        row[:] = 0
        row[0] = len(out)
        row[1: 1 + len(out)] = out
    g[in_d, vb:] = 0
    st = dict(rows=len(cl), removed=int(in_d.sum()), dropped=dropped, still_excluded=len(remaining), affected=np.array(sorted(cl), dtype=np.uint32))
    return dataclasses.replace(ix, graph=g), st, remaining
