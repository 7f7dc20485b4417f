"""Float indexes at the ends of the float range: the same small graphs with their values scaled by powers of two, moved to both signs, or
moved far from zero.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  Every other float input of the suite comes from synth.make_vectors, whose float
vectors are standardised: elements about N(0, 0.28) of both signs, |x| < 1.3, nearest-neighbour distances around 1.  The inputs here are
functions of such an index (ix, q); inside the input domain of DESIGN.md section 2, CANON 20 (finite, |x| <= 2^56) they reach what those
values never do.  tests/test_float_range_inputs.py asserts ON
THE CPU REFERENCES that each reaches the edge it is named for, tests/test_gpu_float_range.py compares every kernel family that reads float
data with its CPU reference on them, bit for bit.

    scaled(ix, q, e)     vectors, pivots, centroid and queries times 2^e (exact: ldexp).  While nothing underflows or overflows every
                         difference, product and sum of the distance chains is the unscaled one times a power of two: ids, counters and
                         candidate log stay, every distance's exponent moves by 2e
      up / down          e = +46 / -46: distances around 2^109 / 2^-75, normal floats far from magnitude 1
      subnormal          e = subnormal_exp(ix, q): at least half of the batch's top-10 exact distances are non-zero SUBNORMALS (the scaled
                         values themselves stay normal).  Low bits are rounded away, so distances tie and order differently than unscaled:
                         no invariant holds, only the oracle's bits
      zero               e = zero_exp(ix, q): every squared difference underflows, every distance is +0 -- the whole walk is ties at zero
    signed(ix, q)        vectors, queries and centroid minus 128.  (The bases already hold both signs, about half of their elements are negative,
                         and up / down scale exactly those; shifted by -128 some 99 % of the elements are negative, at a common magnitude of
                         2^7 with an ulp of 2^-17 against differences of 0.3.)  A sprinkling of -0.0; queries 0 and 1 are bit-copies of an
                         index vector each (the medoid's, one of its neighbours'), and three more neighbours of the medoid are copies of
                         those two vectors: distances of exactly +0 and ties at zero in the seed list of every walk
    offset(ix, q)        vectors, queries and centroid plus 2^20: a large common magnitude (ulp 1/8), small differences
    fp16_straddle        scaled by 2^-12 (FP16_STRADDLE_EXP): elements of N(0, 0.28) lie on both sides of 2^-2, scaled on both sides of fp16's
                         smallest normal 2^-14 (about 60 % below it) -- for the fp16 vector table, whose conversion then produces normal and
                         subnormal halves side by side (expected values: fp16_inputs.rounded of the scaled index).  up / down / subnormal /
                         zero do not apply to that table: fp16 ends at 65504 and 2^-24

    BASES, base()        the smallest float indexes that reach each kernel;  get(base, input) -> (Index, queries)
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from bang_amd.formats import pack_graph

UP_EXP, DOWN_EXP = 46, -46
FP16_STRADDLE_EXP = -12
DOMAIN_MAX = np.float32(2.0 ** 56)
SIGNED_SHIFT = np.float32(128.0)
OFFSET = np.float32(2.0 ** 20)
LS = (10, 37)
K = 10
SCALES = ("up", "down", "subnormal", "zero")
NAMES = SCALES + ("signed", "offset")
INVARIANT = ("up", "down")                   # the scales at which ids stay and distances shift exactly

# name -> where the index comes from.  d68 / d252 / d4: edge_inputs.SHAPES (600 nodes; 12, 8 and 12 queries): one dword past a 64-element
# query register with full rows of R = 64; a partial tail in the fourth register, a layout on the LUT path; a single 16-byte load per vector.
# f32_260: highdim_inputs, the wide exact instances -- and the smallest float entry there on the LUT path.  fp16_256: fp16_inputs.synth_index(256), the one D of that list
# that both the fp16 re-rank and the exact-distance kernel on an fp16 table (D % 8 == 0, D <= 256) take.
BASES = ("d68", "d252", "d4", "f32_260", "fp16_256")
_SHAPE = {"d68": (600, 68, "float", 64, 17, 12), "d252": (600, 252, "float", 64, 63, 8), "d4": (600, 4, "float", 8, 2, 12)}


@functools.lru_cache(maxsize=None)
def base(name: str):
    """-> (Index, queries)"""
    if name in _SHAPE:
        import edge_inputs as E
        assert _SHAPE[name] in E.SHAPES
        return E.shape_index(_SHAPE[name])
    if name == "f32_260":
        import highdim_inputs as H
        return H.get("f32_260")
    if name == "fp16_256":
        import fp16_inputs as FP
        return FP.synth_index(256)
    raise ValueError(name)


def _with(ix, vectors=None, pivots=None, centroid=None):
    v = ix.vectors() if vectors is None else np.ascontiguousarray(vectors, np.float32)
    return dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency()),
                               pivots=ix.pivots if pivots is None else np.ascontiguousarray(pivots, np.float32),
                               centroid=ix.centroid if centroid is None else np.ascontiguousarray(centroid, np.float32))


def _ldexp(a, e: int) -> np.ndarray:
    return np.ldexp(np.asarray(a, np.float32), np.int32(e)).astype(np.float32)


def scaled(ix, q, e: int):
    assert ix.dtype == "float"
    return _with(ix, _ldexp(ix.vectors(), e), _ldexp(ix.pivots, e), _ldexp(ix.centroid, e)), np.ascontiguousarray(_ldexp(q, e))


def shifted_bits(d: np.ndarray, e: int) -> np.ndarray:
    """The bits of d * 2^(2e) for normal results: the exponent field moved by 2e; zeros and the padding sentinel stay."""
    from exact_reference import BIG_DIST
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(over="ignore"):                               # (the sentinel times 2^92)
        out = _ldexp(d, 2 * e)
    out[d == BIG_DIST] = BIG_DIST
    return out.view(np.uint32)


def _all_exact(ix, q) -> np.ndarray:
    """f32 [Q][N]: orc_exact_dist of every node against every query."""
    from exact_reference import Reference
    ref = Reference(ix)
    every = np.arange(int(ix.N), dtype=np.uint32)
    return np.stack([ref.exact(every, np.ascontiguousarray(q[i])) for i in range(q.shape[0])])


def _all_pq(ix, q) -> np.ndarray:
    """f32 [Q][N]: the oracle's PQ distance of every node against every query."""
    from oracle import oracle as O
    orc = O.Oracle(ix)
    every = np.arange(int(ix.N), dtype=np.uint32)
    return np.stack([orc.pqdist(orc.lut_build(np.ascontiguousarray(q[i])), every) for i in range(q.shape[0])])


def top10_exact(ix, q) -> np.ndarray:
    """f32 [Q][10]: the ten smallest exact distances of every query, brute force."""
    return np.sort(_all_exact(ix, q), axis=1)[:, :K]


def exps_of(ix, q):
    """(subnormal e, zero e) of an index and its queries"""
    t = top10_exact(ix, q).astype(np.float64)
    # subnormal floats span 2^-149 .. 2^-126: the median top-10 distance goes to the middle of that span
    sub = int(math.floor((-137.0 - math.log2(float(np.median(t[t > 0])))) / 2.0))
    # the sum of a chain rounds to +0 when it is at most 2^-150 (half the smallest subnormal, ties to even): the largest distance any walk can
    # evaluate -- exact or PQ, any node -- goes below 2^-152
    dmax = max(float(_all_exact(ix, q).max()), float(_all_pq(ix, q).max()))
    zero = int(math.floor((-152.0 - math.ceil(math.log2(dmax))) / 2.0))
    return sub, zero


@functools.lru_cache(maxsize=None)
def _exps(name: str):
    return exps_of(*base(name))


def subnormal_exp(name: str) -> int:
    return _exps(name)[0]


def zero_exp(name: str) -> int:
    return _exps(name)[1]


def exp_of(name: str, scale: str) -> int:
    return {"up": UP_EXP, "down": DOWN_EXP, "subnormal": subnormal_exp(name), "zero": zero_exp(name)}[scale]


def signed(ix, q):
    assert ix.dtype == "float" and q.shape[0] >= 2
    rng = np.random.default_rng(5000 + ix.D)
    v = ix.vectors() - SIGNED_SHIFT
    qq = np.ascontiguousarray(q, np.float32) - SIGNED_SHIFT
    v[rng.random(v.shape) < 0.01] = np.float32(-0.0)
    qq[rng.random(qq.shape) < 0.01] = np.float32(-0.0)
    # The medoid and its neighbours are the seed list: every walk at every L evaluates them.  Query 0 becomes a copy of the medoid's vector and so
    # do the medoid's first two neighbours; query 1 becomes a copy of the third neighbour's vector and so does the fourth neighbour.
    nb = ix.adjacency()[int(ix.medoid)][: int(ix.degrees()[int(ix.medoid)])].astype(np.int64)
    assert len(nb) >= 4 and int(ix.medoid) not in nb[:4] and len(set(nb[:4].tolist())) == 4
    v[nb[0]] = v[nb[1]] = v[int(ix.medoid)]
    v[nb[3]] = v[nb[2]]
    qq[0] = v[int(ix.medoid)]
    qq[1] = v[nb[2]]
    return _with(ix, v, centroid=ix.centroid - SIGNED_SHIFT), np.ascontiguousarray(qq)


def offset(ix, q):
    assert ix.dtype == "float"
    return _with(ix, ix.vectors() + OFFSET, centroid=ix.centroid + OFFSET), np.ascontiguousarray(np.asarray(q, np.float32) + OFFSET)


@functools.lru_cache(maxsize=None)
def get(name: str, what: str):
    """-> (Index, queries) of input `what` (one of NAMES, "unscaled" or "fp16_straddle") on base `name`"""
    ix, q = base(name)
    if what == "unscaled":
        return ix, q
    if what in SCALES:
        return scaled(ix, q, exp_of(name, what))
    if what == "signed":
        return signed(ix, q)
    if what == "offset":
        return offset(ix, q)
    if what == "fp16_straddle":
        return scaled(ix, q, FP16_STRADDLE_EXP)
    raise ValueError(what)


def in_domain(ix, q) -> bool:
    return all(bool((np.abs(a) <= DOMAIN_MAX).all()) for a in (ix.vectors(), ix.pivots, ix.centroid, q))


def is_subnormal(d: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return ((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)
