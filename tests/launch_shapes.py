"""Launch shapes that put the wave-resident search kernels into FULL workgroups, and the table of cases that run in them.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  Every search kernel keeps one query per wave, the wave's lists in its own slice of the
workgroup's LDS, and takes its next query from a hand-out counter.  bang_wave_geometry / bang_search_geometry spread a batch of fewer queries than
CUs x waves over all CUs: the 12 to 64 queries of the other GPU files launch as that many workgroups of ONE wave with one query each.  The shapes
below force what such a launch never has -- neighbours in LDS, and a second query for a wave whose neighbours are still at work:

    shape          BANG_SEARCH_MAX_WGS  BANG_SEARCH_MAX_WAVES  batch                       must reach
    one_workgroup  1                    unset                  32                          1 workgroup of every wave that fits (>= 8), >= 2 queries per wave
    ragged         3                    5                      32                          15 waves, 17 queries through the counter
    full_chip      unset                unset                  full grid x waves + 3       the branch of a batch that fills the chip: the whole grid, full
                                                               (the queries tiled)         workgroups, the rest through the counter

    SHAPES, set_caps()         the caps, and how a test sets them (the engine reads them at launch)
    FAMILIES                   kernel family -> geometry export, engine options, LDS bytes per wave, launch bound
    geometry()                 (workgroups, waves) of a launch from the family's own *_geometry export (needs the device for the wave families)
    full_chip_batch()          the smallest batch that runs the whole grid in full workgroups, from geometry() -- nothing is tied to 256 CUs or 16 waves
    assert_reached()           the "must reach" column, on the pair geometry() returned
    tile(), tile_want(), tile_rows()   a batch made by repeating queries, and the reference's rows repeated the same way
    *_CASES                    the cases of tests/test_gpu_launch_shapes.py; tests/test_launch_shapes.py checks the same list without a GPU
    traces() ...               the CPU references of the existing helper modules, computed once per (input, L) on the BASE queries only
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

NQ = 32                                      # the batch of one_workgroup and ragged
FULL_Q = 100000                              # a batch that fills any chip: geometry(Q = FULL_Q) is the full grid
MIN_WAVES = 8                                # one_workgroup / full_chip: a workgroup of the wave families holds at least this many
MIN_WAVES_SEARCH = 4                         # ... of search_kernel's builds (the pivot table takes most of the LDS): see long_L()
LDS_BYTES = 160 * 1024
MAX_L = 512
OK = 0

Shape = collections.namedtuple("Shape", "max_wgs max_waves")
SHAPES = {"one_workgroup": Shape(1, None), "ragged": Shape(3, 5), "full_chip": Shape(None, None)}


def set_caps(monkeypatch, shape: str):
    s = SHAPES[shape]
    for var, v in (("BANG_SEARCH_MAX_WGS", s.max_wgs), ("BANG_SEARCH_MAX_WAVES", s.max_waves)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))


def caps(shape: str):
    s = SHAPES[shape]
    return s.max_wgs or 0, s.max_waves or 0


# ---------------------------------------------------------------------------------------------------------------------
# LDS bytes per wave, restated from the launchers (csrc/bang_exact_dist.h, bang_search_exact.hip, bang_search_beam.hip, bang_search_lut.hip)
# ---------------------------------------------------------------------------------------------------------------------
SCRATCH_WORDS = 144
TILE_WORDS = 1024


def wl_words(L: int) -> int:
    return (2 * L + (L + 3) // 4 + 3) & ~3


def plain_bytes(L: int, beam: int = 0) -> int:
    return 4 * (wl_words(L) + SCRATCH_WORDS)


def labels_bytes(L: int, beam: int = 0) -> int:
    return 4 * (2 * wl_words(L) + SCRATCH_WORDS)


def wide_bytes(L: int, beam: int = 0) -> int:
    return 4 * (wl_words(L) + SCRATCH_WORDS + TILE_WORDS)


def beam_bytes(L: int, beam: int) -> int:
    return 4 * (wl_words(L) + SCRATCH_WORDS + 2 * (64 * beam + 4))


# ---------------------------------------------------------------------------------------------------------------------
# kernel families
# ---------------------------------------------------------------------------------------------------------------------
# kind: the argument list of the export -- "wave" (dtype, L, Q, caps), "beam" (dtype, L, beam, Q, caps), "lut" (L, Q, caps), "search" (psz, mp, nhi,
# L, Q, caps, host_paced, ..., nctx, group_waves) and "search8" (psz, mp, nhi, L, Q, caps).  wave_bytes: None for search_kernel's builds, whose LDS
# is the pivot table plus the waves (bang_search_supported).  bound(dtype): waves of the instance's launch bound.
Family = collections.namedtuple("Family", "export kind options wave_bytes bound")
_HBM = dict(graph=1, distance=1)
_PULL = dict(graph=0, pull=1, distance=1)


def _b16(dtype):
    return 16


def _wide_bound(dtype):
    return 12 if dtype == "float" else 16      # __launch_bounds__(768) on the float wide instances


FAMILIES = {
    "exact":           Family("bang_search_exact_geometry", "wave", _HBM, plain_bytes, _b16),
    "exact_pull":      Family("bang_search_exact_pull_geometry", "wave", _PULL, plain_bytes, _b16),
    # (the wide builds' geometry functions are exported by the library and declared in csrc/bang_internal.h: bang_k_search_exact routes to them)
    "exact_wide":      Family("bang_search_exact_wide_geometry", "wave", _HBM, wide_bytes, _wide_bound),
    "exact_wide_pull": Family("bang_search_exact_wide_pull_geometry", "wave", _PULL, wide_bytes, _wide_bound),
    "exact_f16":       Family("bang_search_exact_pull_f16_geometry", "wave", dict(_PULL, vectors_fp16=1), plain_bytes, _b16),
    "labels":          Family("bang_search_exact_labels_geometry", "wave", _HBM, labels_bytes, _b16),
    "labels_pull":     Family("bang_search_exact_labels_pull_geometry", "wave", _PULL, labels_bytes, _b16),
    "range":           Family("bang_search_exact_range_geometry", "wave", _HBM, plain_bytes, _b16),
    "range_pull":      Family("bang_search_exact_range_pull_geometry", "wave", _PULL, plain_bytes, _b16),
    "beam":            Family("bang_search_exact_beam_geometry", "beam", _HBM, beam_bytes, _b16),
    "beam_pull":       Family("bang_search_exact_beam_pull_geometry", "beam", _PULL, beam_bytes, _b16),
    "lut":             Family("bang_search_lut_geometry", "lut", dict(graph=1, search=1), plain_bytes, _b16),
    # search_kernel: the engine options are those of a form of tests/base_forms.py
    "search":          Family("bang_search_geometry", "search", None, None, None),
    "inmemory":        Family("bang_search_inmem_geometry", "search8", dict(graph=1, semantics=1), None, None),
    "wordfilter":      Family("bang_search_wf_geometry", "search8", dict(filter_layout=1), None, None),
}
INTERNAL_EXPORTS = ("bang_search_exact_wide_geometry", "bang_search_exact_wide_pull_geometry")

# input -> dtype (conftest's fixtures; tests/highdim_inputs.py)
NARROW = {"small_u8": "uint8", "small_i8": "int8", "small_f32": "float", "small_deep": "float"}
WIDE = {"mnist_like": "uint8", "i8_1024": "int8", "gist_like": "float", "f32_260": "float", "u8_48": "uint8"}


def _lib():
    from bang_amd import binding as B
    return B.lib()


def dtype_code(dtype: str) -> int:
    from bang_amd import binding as B
    return B.DTYPE_CODE[dtype]


def _pq_layout(ix, pq_ragged: int):
    """(psz, mp, the NHI of the exact-size pivot table or 0): bang_load.cpp offers the table where an instance exists for it"""
    from bang_amd import binding as B
    lib = _lib()
    lib.bang_ragged_supported.argtypes = [C.c_uint32] * 4
    psz, mp = B.pq_layout(ix.chunk_off, ix.D, ix.m)
    nhi = 0
    if psz == 2 and pq_ragged:
        nhi, _ = B.pack_pivots_ragged(ix.pivots, ix.chunk_off, ix.D, ix.m, mp)
        if not (nhi and lib.bang_ragged_supported(psz, mp, nhi, ix.m)):
            nhi = 0
    return int(psz), int(mp), int(nhi)


def _waves_that_fit(psz, mp, nhi, L):
    lib = _lib()
    lib.bang_search_supported.argtypes = [C.c_uint32] * 4
    return int(lib.bang_search_supported(psz, mp, nhi, L))


def pq_args(ix, L: int, pq_ragged: int = 1):
    """(psz, mp, nhi) of a search_kernel launch on this index at this L, decided as bang_load.cpp and bang_alloc.cpp decide it: the exact-size pivot
    table where it is offered and leaves LDS for more waves than the padded one (tests/test_instance_inputs.py pins the rule)."""
    psz, mp, nhi = cached(("pq_layout", id(ix), pq_ragged), lambda: _pq_layout(ix, pq_ragged))
    w_pad = _waves_that_fit(psz, mp, 0, L)
    w_rag = _waves_that_fit(psz, mp, nhi, L) if nhi else 0
    return psz, mp, (nhi if w_rag > w_pad else 0)


def long_L(ix, pq_ragged: int = 1, inmemory: bool = False) -> int:
    """The longest worklist <= 512 at which a workgroup of search_kernel on this layout still holds MIN_WAVES_SEARCH waves.  bang_search_supported
    admits every layout of tests/instance_inputs.py at L = 512, some with one or two waves beside the pivot table: that is the one-wave launch again,
    and below four waves bang_alloc declines the pulled form under search = auto.  Four is that threshold.
    inmemory: the Inmemory build logs up to L + 120 candidates, and where the fused re-rank does not evaluate the layout the engine refuses a log
    of more than 512 + 50 (the separate re-rank launch): L <= 442 there."""
    top = MAX_L
    if inmemory:
        fn = _lib().bang_search_can_rerank
        fn.argtypes, fn.restype = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32], C.c_int
        if not fn(dtype_code(ix.dtype), int(ix.D), int(ix.entry_len), 0):
            top = MAX_L + 50 - 120
    for L in range(top, 0, -1):
        if _waves_that_fit(*pq_args(ix, L, pq_ragged), L) >= MIN_WAVES_SEARCH:
            return L
    raise AssertionError("no worklist length leaves room for four waves")


def geometry(family: str, L: int, Q: int, shape: str, dtype: str | None = None, beam: int = 0, pq=None):
    """(workgroups, waves) of the launch the engine makes: the family's own export, with the caps of `shape`.  pq = pq_args(...) for search_kernel."""
    f = FAMILIES[family]
    fn = getattr(_lib(), f.export)
    u32, ptr = C.c_uint32, C.POINTER(C.c_uint32)
    wg, wv, nctx, gs = u32(0), u32(0), u32(0), u32(0)
    max_wgs, max_waves = caps(shape)
    tail = [(u32, Q), (u32, max_wgs), (u32, max_waves)]
    out = [(ptr, C.byref(wg)), (ptr, C.byref(wv))]
    if f.kind == "wave":
        args = [(C.c_int, dtype_code(dtype)), (u32, L)] + tail + out
    elif f.kind == "beam":
        args = [(C.c_int, dtype_code(dtype)), (u32, L), (u32, beam)] + tail + out
    elif f.kind == "lut":
        args = [(u32, L)] + tail + out
    elif f.kind == "search":
        args = [(u32, x) for x in pq] + [(u32, L)] + tail + [(C.c_int, 0)] + out + [(ptr, C.byref(nctx)), (ptr, C.byref(gs))]
    else:
        args = [(u32, x) for x in pq] + [(u32, L)] + tail + out
    fn.restype = C.c_int
    fn.argtypes = [t for t, _ in args]
    rc = fn(*(v for _, v in args))
    assert rc == OK, (family, f.export, rc)
    return int(wg.value), int(wv.value)


def rounds_of(family: str) -> int:
    """Wave-fulls of a full_chip batch.  bang_wave_geometry runs full workgroups as soon as a batch exceeds one wave-full; bang_search_geometry runs a
    batch of one to two wave-fulls as two equal rounds of HALF the waves, so search_kernel's builds are full from two wave-fulls on."""
    return 2 if FAMILIES[family].kind in ("search", "search8") else 1


def full_chip_batch(family: str, L: int, **kw):
    """-> (Q, (workgroups, waves)): the full grid of the family at this L, and the batch that fills it rounds_of() times and leaves 3 queries"""
    wg, wv = geometry(family, L, FULL_Q, "full_chip", **kw)
    return rounds_of(family) * wg * wv + 3, (wg, wv)


def assert_reached(shape: str, got, Q: int, full, min_waves: int = MIN_WAVES, rounds: int = 1):
    """got = geometry(..., Q, shape); full = geometry(..., FULL_Q, "full_chip"): the uncapped grid"""
    wg, wv = got
    what = (shape, got, Q, full)
    if shape == "one_workgroup":
        assert wg == 1 and wv == full[1] and wv >= min_waves and Q >= 2 * wv, what      # every wave that fits, each with a second query
    elif shape == "ragged":
        assert (wg, wv) == (3, 5) and full[1] >= 5 and Q - wg * wv == 17, what
    elif shape == "full_chip":
        assert got == full and wv >= min_waves and Q == rounds * wg * wv + 3 and Q < FULL_Q, what
    else:
        raise ValueError(shape)


# ---------------------------------------------------------------------------------------------------------------------
# batches made of repeated queries
# ---------------------------------------------------------------------------------------------------------------------
def _index(n: int, Q: int) -> np.ndarray:
    return np.arange(Q) % n


def tile(q: np.ndarray, Q: int) -> np.ndarray:
    """Q queries: the rows of q in turn, again and again.  A copy of a query must return the bits of the original."""
    return np.ascontiguousarray(q[_index(q.shape[0], Q)])


def tile_rows(rows, Q: int):
    """a per-query list (traces, radii, ...) repeated as tile() repeats the queries"""
    if isinstance(rows, np.ndarray):
        return np.ascontiguousarray(rows[_index(rows.shape[0], Q)])
    return [rows[i] for i in _index(len(rows), Q)]


def tile_want(want, Q: int):
    """A reference result (ids [n][k], dists [k][n] rank-major, then any number of per-query arrays [n][...]) repeated as tile() repeats the queries"""
    ids, d = want[0], want[1]
    ix = _index(ids.shape[0], Q)
    return (np.ascontiguousarray(ids[ix]), np.ascontiguousarray(d[:, ix])) + tuple(np.ascontiguousarray(np.asarray(a)[ix]) for a in want[2:])


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# (shape, L, k): full workgroups and the ragged grid at the L of the other files' launch-shape tests, and the fullest LDS with the whole list compared
RUNS = (("one_workgroup", 37, 10), ("ragged", 37, 10), ("one_workgroup", MAX_L, MAX_L))
FULL_L, FULL_K = 37, 10


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# (family, input, shape, L, k)
EXACT_CASES = ([(fam, name) + run for name in NARROW for fam in ("exact", "exact_pull") for run in RUNS] +
               [(fam, name) + run for name in WIDE for fam in ("exact_wide", "exact_wide_pull") for run in RUNS] +
               [("exact_f16", "small_deep") + run for run in RUNS])
LABEL_INPUTS = ("small_u8", "small_f32", "small_i8")
# (family, input, shape, L, k, extra): extra = "plain" | "excluded" | "lanes2"
LABELS_CASES = ([(fam, name) + run + ("plain",) for name in LABEL_INPUTS for fam in ("labels", "labels_pull") for run in RUNS] +
                [(fam, "small_u8", "one_workgroup", 37, 10, extra) for fam in ("labels", "labels_pull") for extra in ("excluded", "lanes2")])
RANGE_CASES = ([(fam, name) + run + ("plain",) for name in LABEL_INPUTS for fam in ("range", "range_pull") for run in RUNS] +
               [(fam, "small_u8", "one_workgroup", 37, 10, extra) for fam in ("range", "range_pull") for extra in ("excluded", "lanes2")])
RANGE_RADII = (("mixed", 512), ("mixed", 64), ("rank400", 512), ("rank400", 64))      # (radii of tests/range_inputs.py, capacity); 64 truncates
# (family, beam): one_workgroup at L = 512, k = L on tie_heavy(small_u8) with 32 queries
BEAM_CASES = [(fam, beam) for fam in ("beam", "beam_pull") for beam in (2, 4)]
SEARCH_FORMS = ("self", "pull_host")            # self: self_fused, or self_launch where the fused re-rank does not evaluate the layout
SEARCH_RUNS = (("one_workgroup", 37), ("ragged", 37), ("one_workgroup", "long"))      # "long": long_L() of the entry
LUT_INPUTS = ("gist_like", "small_u8")          # a natural LUT layout; pq = 1 forced on a fixture
# (family, input): full_chip at L = 37, k = 10
FULL_CASES = [("exact", "small_u8"), ("exact_pull", "small_u8"), ("labels", "small_u8"), ("range", "small_u8"), ("beam", "small_u8"),
              ("search", "small_u8"), ("inmemory", "small_u8"), ("wordfilter", "small_u8"), ("exact_wide", "gist_like"), ("exact_f16", "small_deep")]
FULL_BEAM = 2
FULL_RANGE = ("mixed", 64)


def input_dtype(name: str) -> str:
    return NARROW[name] if name in NARROW else WIDE[name]


def wave_cases():
    """Every (family, dtype, L, shape, beam) that tests/test_gpu_launch_shapes.py launches on a kernel whose grid is bang_wave_geometry's"""
    out = set()
    for fam, name, shape, L, _ in EXACT_CASES:
        out.add((fam, input_dtype(name), L, shape, 0))
    for fam, name, shape, L, _, _ in LABELS_CASES + RANGE_CASES:
        out.add((fam, input_dtype(name), L, shape, 0))
    for fam, beam in BEAM_CASES:
        out.add((fam, "uint8", MAX_L, "one_workgroup", beam))
    for name in LUT_INPUTS:
        out.add(("lut", input_dtype(name), MAX_L, "one_workgroup", 0))
    for fam, name in FULL_CASES:
        if FAMILIES[fam].kind not in ("search", "search8"):
            out.add((fam, input_dtype(name), FULL_L, "full_chip", FULL_BEAM if fam == "beam" else 0))
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references, from the existing helper modules; the references run on the base queries, once per (input, L)
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def load_input(name: str, fixture):
    """-> (index, base queries: at most NQ).  fixture = request.getfixturevalue for conftest's indexes"""
    if name in NARROW:
        ix, q = fixture(name)[:2]
    else:
        import highdim_inputs as H
        ix, q = H.get(name)
    return ix, np.ascontiguousarray(q[:NQ])


def tie_heavy32(fixture):
    import edge_inputs as E
    return cached(("tie_heavy", NQ), lambda: E.tie_heavy(*fixture("small_u8")[:2], n_queries=NQ))


def reference_index(family: str, ix):
    """The index the CPU reference walks: for fp16 rows the copy whose vectors are rounded to fp16 (tests/fp16_inputs.py)"""
    if family == "exact_f16":
        import fp16_inputs as FP
        return cached(("rounded", id(ix)), lambda: FP.rounded(ix))
    return ix


def traces(key, ix, q, L):
    """labels_reference.Reference.walks: the exact-distance walk with final worklist, counters, candidate log and the merged survivors"""
    import labels_reference as LR
    return cached(("walks", key, q.shape, L), lambda: LR.Reference(ix).walks(q, L))


def range_traces(key, ix, q, L):
    import range_reference as RR
    return cached(("evaluated", key, q.shape, L), lambda: RR.Reference(ix).evaluated_all(q, L))


def range_reference(key, ix):
    import range_reference as RR
    return cached(("range_ref", key), lambda: RR.Reference(ix))


def beam_reference(key, ix, q, L, beam):
    from beam_reference import Reference
    return cached(("beam", key, q.shape, L, beam), lambda: Reference(ix).search(q, L, L, beam))


def oracle_reference(key, ix, q, k, L):
    from oracle import oracle as O
    return cached(("oracle", key, q.shape, k, L), lambda: O.Oracle(ix).search(q, k, L, with_stats=True))


def inmemory_reference(key, ix, q, k, L):
    from inmemory_reference import Reference
    return cached(("inmemory", key, q.shape, k, L), lambda: Reference(ix).search(q, k, L, "inmemory"))


def wordfilter_reference(key, ix, q, k, L):
    import wordfilter_reference as W
    return cached(("word", key, q.shape, k, L), lambda: W.Reference(ix).search(q, k, L, "word"))


def from_traces(trs, k: int):
    """-> (ids u64 [Q][k], dists f32 [k][Q], stats [Q][4], logs: list of u32 arrays): the first k worklist entries, padded"""
    import labels_reference as LR
    Q = len(trs)
    ids = np.full((Q, k), LR.PAD_ID, np.uint64)
    d = np.full((k, Q), LR.BIG_DIST, np.float32)
    st = np.empty((Q, 4), np.int64)
    for i, t in enumerate(trs):
        n = min(k, len(t.wl_ids))
        ids[i, :n] = t.wl_ids[:n]
        d[:n, i] = t.wl_dists[:n]
        st[i] = t.stats
    return ids, d, st, [t.log for t in trs]
