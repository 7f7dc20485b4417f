"""Small indexes on which the two visited-filter layouts (option ``filter_layout``: split | word) DISAGREE.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  On an ordinary small fixture a query touches a few thousand of the filter's
400 384 bits and neither layout ever drops an id it has not seen: the layouts give the same results, and a kernel that ignored the option would
pass every comparison.  The inputs here force the layouts apart with ids whose filter positions collide.  The collisions are searched among the
ids below N with the oracle's own hashes (``collisions``; nothing is taken from a table), and a search that finds none raises.  Every input is a
``synth.make_index`` index (N = 8192, D = 32, uint8, m = 8: the 4-dimension-chunk layout with 16 padded chunks) whose nodes are RELABELLED --
vectors, codes, adjacency ids and the medoid permuted together, rows sorted ascending again -- so that the colliding ids sit where query 0 meets
them in the order that matters: the earlier ones in the seed list (the medoid's row: survivors of iteration 1), the later one in the row of a
parent expanded afterwards.  Each builder then runs both references (tests/wordfilter_reference.py) on query 0 and raises unless the stated id
is dropped by the stated layout in the stated iteration and evaluated by the other.

    word_drops()        a, then c: c's mask lies inside a's (same word).  The word layout drops c; the split layout evaluates it.
    split_drops()       a1, a2, then c: hash1(c) and hash2(c) are positions a1 and a2 set.  The split layout drops c; the word layout evaluates it.
    shared_word_row()   u and v, both fresh, share a filter word IN ONE ROW (both are kept, both masks must land in the word); then w, whose mask
                        needs bits of both.  The word layout drops w only if the two masks were merged into one store.
    one_bit()           a, then z: z's two positions coincide (a one-bit mask) and a sets that bit.  The word layout drops z.
    seed65()            a medoid of degree 64 (R = 64): a seed list of 65 ids.  u is among the first 64, v is the 65th -- the id a wave's 64 lanes do
                        not hold -- and they share a word; w's mask needs bits of both.
    INPUTS              name -> builder;  each returns Input(ix, q, query, iteration, id, dropped_by)
"""
from __future__ import annotations

import collections
import dataclasses
import functools

import numpy as np

from bang_amd import synth
from bang_amd.formats import pack_graph

import wordfilter_reference as W

N, D, DTYPE, M, Q = 8192, 32, "uint8", 8, 6
L_TRACE = 10
Input = collections.namedtuple("Input", "ix q query iteration id dropped_by")
Collisions = collections.namedtuple("Collisions", "word_only split_only shared_word one_bit one_bit_drop")


def _bits(x: int) -> int:
    return bin(x).count("1")


@functools.lru_cache(maxsize=None)
def collisions(n: int = N) -> Collisions:
    """The colliding ids below n, from the oracle's hashes.
    word_only (a, c): same word, mask(c) inside mask(a), and a alone does not set both split positions of c.
    split_only (a1, a2, c): hash1(c) is a position of a1, hash2(c) one of a2, and a1, a2 do not cover mask(c) in c's word.
    shared_word (u, v, w): one word; mask(w) inside mask(u) | mask(v) but inside neither.
    one_bit: ids whose two word-local positions coincide;  one_bit_drop (a, z): z one-bit, same word, its bit in mask(a)."""
    words, pos = collections.defaultdict(list), collections.defaultdict(list)
    for x in range(n):
        a, b = W.positions(x)
        words[a >> 5].append(x)
        pos[a].append(x)
        pos[b].append(x)
    mask, word = W.mask_of, W.word_of
    word_only = [(a, c) for ids in words.values() for a in ids for c in ids
                 if a != c and mask(c) & ~mask(a) == 0 and not (W.positions(c)[0] in W.positions(a) and W.positions(c)[1] in W.positions(a))]
    split_only = []
    for c in range(n):
        h1, h2 = W.positions(c)
        for a1 in pos[h1]:
            for a2 in pos[h2]:
                if c in (a1, a2):
                    continue
                covered = 0
                for a in {a1, a2}:
                    if word(a) == word(c):
                        covered |= mask(a)
                if mask(c) & ~covered:
                    split_only.append((a1, a2, c))
    shared = [(u, v, w) for ids in words.values() if len(ids) >= 3 for u in ids for v in ids for w in ids
              if u < v and w not in (u, v) and mask(w) & ~(mask(u) | mask(v)) == 0 and mask(w) & ~mask(u) and mask(w) & ~mask(v)]
    one_bit = [x for x in range(n) if _bits(mask(x)) == 1]
    one_bit_drop = [(a, z) for z in one_bit for a in words[word(z)] if a != z and mask(z) & ~mask(a) == 0]
    found = Collisions(sorted(word_only), sorted(split_only), sorted(shared), one_bit, sorted(one_bit_drop))
    for name, ids in found._asdict().items():
        if not ids:
            raise RuntimeError(f"wordfilter_inputs: no '{name}' collision among the ids below {n}: the crafted inputs cannot be built")
    return found


@functools.lru_cache(maxsize=None)
def base_index(R: int = 32):
    ix, q, _, _ = synth.make_index(N, D, DTYPE, R, M, Q, K=10, n_clusters=32, seed=4100 + R, device="cpu", pq_iters=2)
    return ix, q


def with_medoid_degree(ix, degree: int):
    """The medoid's row filled up to `degree` ids with neighbours of its neighbours."""
    deg, adj = ix.degrees().copy(), ix.adjacency().copy()
    m = int(ix.medoid)
    row = [int(x) for x in adj[m][:deg[m]]]
    for n1 in list(row):
        for x in adj[n1][:deg[n1]]:
            if len(row) < degree and int(x) != m and int(x) not in row:
                row.append(int(x))
    assert len(row) == degree <= ix.R
    deg[m] = degree
    adj[m][:degree] = sorted(row)
    return dataclasses.replace(ix, graph=pack_graph(ix.vectors(), deg, adj))


def relabel(ix, pins):
    """Node `old` becomes node `new` for every (old, new) of pins; the node that was `new` takes the label that is freed.  Vectors, codes,
    adjacency ids and the medoid move together; every row is sorted ascending again."""
    perm = np.arange(ix.N)                       # old label -> new label
    inv = np.arange(ix.N)                        # new label -> old label
    pinned = set()
    for old, new in pins:
        other = int(inv[new])                    # the node that holds the wanted label now
        if other == old:
            pinned.add(old)
            continue
        if other in pinned or old in pinned:
            raise RuntimeError(f"wordfilter_inputs.relabel: pins collide at ({old}, {new})")
        freed = int(perm[old])
        perm[old], perm[other] = new, freed
        inv[new], inv[freed] = old, other
        pinned.add(old)
    assert np.array_equal(np.sort(perm), np.arange(ix.N))
    deg, adj, vec = ix.degrees(), ix.adjacency(), ix.vectors()
    deg2, adj2, vec2, codes2 = np.empty_like(deg), np.zeros_like(adj), np.empty_like(vec), np.empty_like(ix.codes)
    for i in range(ix.N):
        j = perm[i]
        deg2[j] = deg[i]
        adj2[j][:deg[i]] = np.sort(perm[adj[i][:deg[i]]])
        vec2[j] = vec[i]
        codes2[j] = ix.codes[i]
    return dataclasses.replace(ix, medoid=int(perm[ix.medoid]), graph=pack_graph(vec2, deg2, adj2), codes=codes2)


def walk(ix, query):
    """What a query meets first under the split layout: (seed list, [parent 1, its row], [parent 2, its row], parent 3)."""
    ref, log = W.Reference(ix), []
    ref.search_one(query, 10, L_TRACE, "split", log=log)
    if len(log) < 4:
        return None
    seed = [int(ix.medoid)] + [int(x) for x in ref.adjacency(int(ix.medoid))]
    return seed, (log[1], [int(x) for x in ref.adjacency(log[1])]), (log[2], [int(x) for x in ref.adjacency(log[2])]), log[3]


def _verify(ix, q, query: int, iteration: int, x: int, dropped_by: str) -> Input:
    """Both references on the query: `x` is offered to the filter in `iteration`, dropped there by `dropped_by` and evaluated by the other
    layout -- and, x being the node the walk would expand next, the two candidate logs part."""
    ref, logs = W.Reference(ix), []
    for layout in W.LAYOUTS:
        trace, log = [], []
        ref.search_one(q[query], 10, L_TRACE, layout, trace=trace, log=log)
        logs.append(log)
        offered = [(t, s) for it, t, s in trace if it == iteration]
        if not offered or x not in offered[0][0]:
            raise RuntimeError(f"wordfilter_inputs: id {x} is not offered in iteration {iteration} under {layout}")
        if (x in offered[0][1]) != (layout != dropped_by):
            raise RuntimeError(f"wordfilter_inputs: id {x} in iteration {iteration} under {layout}: expected it "
                               f"{'dropped' if layout == dropped_by else 'evaluated'}")
    if logs[0] == logs[1]:
        raise RuntimeError(f"wordfilter_inputs: dropping id {x} does not change the candidate log")
    return Input(ix, q, query, iteration, x, dropped_by)


def _fresh(row, *seen):
    """The nodes of a row that none of the earlier rows holds."""
    taken = set().union(*[set(s) for s in seen])
    return [x for x in row if x not in taken]


def _place(R: int, seed_ids, row1_ids, row2_ids=(), dropped_by="word", medoid_degree=None, last_seed=None):
    """Relabel the base index so that, for one of its queries, seed_ids are neighbours of the medoid, row1_ids fresh ids of the first parent's
    row and row2_ids fresh ids of the second parent's.  The last id of row1_ids / row2_ids is the one the layouts disagree on: it goes to the
    node the query expands NEXT (so that dropping it changes the walk, not only a counter).  last_seed: that id must be the LAST of the seed
    list, i.e. the largest label in the medoid's row -- neighbours with larger labels are moved below it."""
    ix, q = base_index(R)
    if medoid_degree:
        ix = with_medoid_degree(ix, medoid_degree)
    special = set(seed_ids) | set(row1_ids) | set(row2_ids)
    for query in range(q.shape[0]):
        met = walk(ix, q[query])
        if met is None:
            continue
        seed, (p1, row1), (p2, row2), p3 = met
        nxt = p3 if row2_ids else p2                                # the node the target id goes to
        f1 = _fresh(row1, seed)
        f2 = _fresh(row2, seed, row1, [p1])
        if nxt not in (f2 if row2_ids else f1):
            continue
        n_seed = [x for x in seed[1:] if x not in (p1, p2, p3)]
        f1 = [x for x in f1 if x not in (p2, p3)]
        f2 = [x for x in f2 if x != p3]
        pins = list(zip(n_seed, seed_ids))
        if row2_ids:
            pins += list(zip(f1, row1_ids)) + list(zip(f2, row2_ids[:-1])) + [(nxt, row2_ids[-1])]
            enough = len(f1) >= len(row1_ids) and len(f2) >= len(row2_ids) - 1
        else:
            pins += list(zip(f1, row1_ids[:-1])) + [(nxt, row1_ids[-1])]
            enough = len(f1) >= len(row1_ids) - 1
        if len(n_seed) < len(seed_ids) or not enough:
            continue
        ix2 = relabel(ix, pins)
        if last_seed is not None:                                   # second pass: nothing but last_seed at or above it in the medoid's row
            row = [int(x) for x in W.Reference(ix2).adjacency(int(ix2.medoid))]
            keep = special | set(row) | {int(ix2.medoid)}
            spare = (x for x in range(last_seed) if x not in keep)
            ix2 = relabel(ix2, [(x, next(spare)) for x in row if x > last_seed])
        return _verify(ix2, q, query, 3 if row2_ids else 2, (row2_ids or row1_ids)[-1], dropped_by)
    raise RuntimeError("wordfilter_inputs: no query of the base index expands a fresh id of the row the collision belongs in")


@functools.lru_cache(maxsize=None)
def word_drops() -> Input:
    a, c = collisions().word_only[0]
    return _place(32, [a], [c], dropped_by="word")


@functools.lru_cache(maxsize=None)
def split_drops() -> Input:
    a1, a2, c = collisions().split_only[0]
    return _place(32, [a1, a2] if a1 != a2 else [a1], [c], dropped_by="split")


@functools.lru_cache(maxsize=None)
def shared_word_row() -> Input:
    u, v, w = collisions().shared_word[0]
    return _place(32, [], [u, v], [w], dropped_by="word")


@functools.lru_cache(maxsize=None)
def one_bit() -> Input:
    a, z = [p for p in collisions().one_bit_drop if p != collisions().word_only[0]][0]          # (not the pair word_drops() uses)
    return _place(32, [a], [z], dropped_by="word")


@functools.lru_cache(maxsize=None)
def seed65() -> Input:
    u, v, w = collisions().shared_word[0]
    inp = _place(64, [u, v], [w], dropped_by="word", medoid_degree=64, last_seed=v)
    row = W.Reference(inp.ix).adjacency(int(inp.ix.medoid))
    if len(row) != 64 or int(row[-1]) != v or u not in row:
        raise RuntimeError("wordfilter_inputs.seed65: the 65th seed id is not the colliding one")
    return inp


INPUTS = {"word_drops": word_drops, "split_drops": split_drops, "shared_word_row": shared_word_row, "one_bit": one_bit, "seed65": seed65}
