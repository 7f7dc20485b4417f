"""tests/launch_shapes.py without a GPU: that every (family, L, shape) of tests/test_gpu_launch_shapes.py reaches the launch it is named for and fits
LDS.  bang_wave_geometry (csrc/bang_wave_host.cpp) is arithmetic alone; on the device the *_geometry exports hand it the kernel's register count
and launch bound.  Here it gets the LDS bytes per wave, restated from the launchers, and every register figure a build could plausibly have
(allocations of 96 .. 136 in granules of 8; today's builds: 104 narrow, 120 label filters, up to 136 wide).  search_kernel's builds (bang_search_geometry: host
arithmetic too) are asked through their own exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instance_inputs as I
import launch_shapes as S
import wordfilter_inputs as WI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
CUS = 256                                    # bang_wave_geometry takes the number of CUs as an argument: any chip of at least NQ CUs shows the same
REGS = tuple(range(96, 137, 8))


def wave_geometry(libbang, regs, bound, nbytes, Q, shape, cus=CUS):
    f = libbang.bang_wave_geometry
    f.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)] * 2
    f.restype = C.c_int
    wg, w = C.c_uint32(0), C.c_uint32(0)
    max_wgs, max_waves = S.caps(shape)
    assert f(regs, bound, nbytes, cus, Q, max_wgs, max_waves, C.byref(wg), C.byref(w)) == OK
    return wg.value, w.value


def test_the_restated_lds_sizes():
    assert S.wl_words(512) == 1152 and S.wl_words(37) == 84
    assert S.plain_bytes(512) == 5184 and S.labels_bytes(512) == 9792 and S.wide_bytes(512) == 9280
    assert S.beam_bytes(512, 2) == 6240 and S.beam_bytes(512, 4) == 7264
    src = open(os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_search_exact.hip")).read()
    assert "#define EXACT_TILE_WORDS 1024u" in src and "#define EXACT_LISTS 2u" in src
    hdr = open(os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_exact_dist.h")).read()
    assert "#define WAVE_SCRATCH_WORDS 144u" in hdr
    assert "(DT) == BANG_F32 ? 768 : 1024" in src                             # the float wide builds: 12 waves


def test_label_filters_at_the_longest_worklist_fill_lds(libbang):
    """The tight case: two lists of capacity 512 per wave, 120 allocated registers -> 16 waves of 9 792 bytes = 156 672 of the 163 840 bytes of a CU"""
    for regs in (114, 118, 120):
        assert wave_geometry(libbang, regs, 16, S.labels_bytes(512), S.NQ, "one_workgroup") == (1, 16)
    assert 16 * S.labels_bytes(512) == 156672 <= S.LDS_BYTES < 17 * S.labels_bytes(512)


@pytest.mark.parametrize("family,dtype,L,shape,beam", S.wave_cases(), ids=S._ids(S.wave_cases()))
def test_every_wave_case_reaches_its_shape(libbang, family, dtype, L, shape, beam):
    fam = S.FAMILIES[family]
    nbytes, bound = fam.wave_bytes(L, beam), fam.bound(dtype)
    reached = 0
    for regs in REGS:
        full = wave_geometry(libbang, regs, bound, nbytes, S.FULL_Q, "full_chip")
        per_cu = min(4 * min(512 // regs, 8), S.LDS_BYTES // nbytes, 32)
        assert full[1] == min(per_cu, 16, bound) and full[0] == CUS * (per_cu // full[1])
        assert full[1] * nbytes <= S.LDS_BYTES, (regs, full)
        Q = S.NQ if shape != "full_chip" else full[0] * full[1] + 3
        got = wave_geometry(libbang, regs, bound, nbytes, Q, shape)
        assert got[1] * nbytes <= S.LDS_BYTES, (regs, got)
        if per_cu >= S.MIN_WAVES:
            S.assert_reached(shape, got, Q, full)
            assert wave_geometry(libbang, regs, bound, nbytes, S.NQ, "full_chip") == (S.NQ, 1)      # the default launch of the other files
            reached += 1
    assert reached == len(REGS)                                               # (at these sizes every figure leaves room for eight waves)


def _search_entries():
    out = [("search", I.entry_id(e), e) for e in I.ENTRIES]
    out += [("inmemory", I.entry_id(e), e) for e in I.ENTRIES if not (e.key == 132 and not I.aligned(e))]
    return out


@pytest.mark.parametrize("family,eid,entry", _search_entries(), ids=lambda v: v if isinstance(v, str) else "")
def test_search_kernel_cases_reach_their_shapes(libbang, family, eid, entry):
    ix, _ = I.entry_index(entry)
    long_L = S.long_L(ix, entry.pq_ragged, inmemory=family == "inmemory")
    assert 37 < long_L <= S.MAX_L
    for shape, L in S.SEARCH_RUNS:
        L = long_L if L == "long" else L
        pq = S.pq_args(ix, L, entry.pq_ragged)
        full = S.geometry(family, L, S.FULL_Q, "full_chip", pq=pq)
        S.assert_reached(shape, S.geometry(family, L, S.NQ, shape, pq=pq), S.NQ, full, S.MIN_WAVES_SEARCH)
        assert S.geometry(family, L, S.NQ, "full_chip", pq=pq) == (S.NQ, 1)
    if long_L < S.MAX_L and long_L != S.MAX_L + 50 - 120:                      # one step further a workgroup holds fewer than four waves
        pq = S.pq_args(ix, long_L + 1, entry.pq_ragged)
        assert S.geometry(family, long_L + 1, S.FULL_Q, "full_chip", pq=pq)[1] < S.MIN_WAVES_SEARCH


@pytest.mark.parametrize("name", list(WI.INPUTS))
def test_wordfilter_cases_reach_their_shapes(libbang, name):
    ix = WI.INPUTS[name]().ix
    for shape, L in S.SEARCH_RUNS:
        L = S.long_L(ix) if L == "long" else L
        pq = S.pq_args(ix, L)
        full = S.geometry("wordfilter", L, S.FULL_Q, "full_chip", pq=pq)
        S.assert_reached(shape, S.geometry("wordfilter", L, S.NQ, shape, pq=pq), S.NQ, full, S.MIN_WAVES_SEARCH)


@pytest.mark.parametrize("family", ("search", "inmemory", "wordfilter"))
def test_full_chip_batch_of_the_search_kernel_builds(libbang, small_u8, family):
    """Two wave-fulls and three: one wave-full and three would run as two rounds of half the waves (bang_search_geometry)"""
    ix = small_u8[0]
    pq = S.pq_args(ix, S.FULL_L)
    Q, full = S.full_chip_batch(family, S.FULL_L, pq=pq)
    S.assert_reached("full_chip", S.geometry(family, S.FULL_L, Q, "full_chip", pq=pq), Q, full, S.MIN_WAVES_SEARCH, 2)
    assert S.geometry(family, S.FULL_L, full[0] * full[1] + 3, "full_chip", pq=pq)[1] < full[1]


def test_tiling_round_trips():
    """A reference computed row by row on the tiled batch is the tiled reference of the base batch"""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 255, (12, 16)).astype(np.uint8)

    def reference(qq, k=3):
        n = qq.shape[0]
        ids = (qq[:, :k].astype(np.uint64) * 7 + 1)
        d = np.ascontiguousarray(qq[:, k:2 * k].T.astype(np.float32))
        st = qq[:, :4].astype(np.int64)
        logs = np.zeros((n, 5), np.uint32) + qq[:, :1]
        return ids, d, st, logs

    for Q in (12, 32, 37):
        t = S.tile(q, Q)
        assert t.shape == (Q, 16) and t.flags["C_CONTIGUOUS"] and np.array_equal(t[:12], q) and np.array_equal(t[12:24], q[:Q - 12][:12])
        got, want = S.tile_want(reference(q), Q), reference(t)
        assert len(got) == len(want) and all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(got, want))
        assert S.tile_rows(list(range(12)), Q) == [i % 12 for i in range(Q)]
        assert np.array_equal(S.tile_rows(np.arange(12), Q), np.arange(Q) % 12)
    assert np.array_equal(S.tile_want(S.tile_want(reference(q), 32), 12)[0], reference(q)[0])


def test_every_family_names_a_declared_geometry_export(libbang):
    """include/bang_c.h declares the export of every family; the two wide builds' are the library's own (csrc/bang_internal.h), reached through
    bang_k_search_exact"""
    public = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    internal = open(os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_internal.h")).read()
    used = {c[0] for c in S.EXACT_CASES + S.LABELS_CASES + S.RANGE_CASES + S.BEAM_CASES + S.FULL_CASES} | {"lut", "search", "inmemory", "wordfilter"}
    assert used == set(S.FAMILIES)
    for name, fam in S.FAMILIES.items():
        header = internal if fam.export in S.INTERNAL_EXPORTS else public
        assert re.search(r"\bint\s+" + fam.export + r"\s*\(", header), (name, fam.export)
        assert (fam.export in S.INTERNAL_EXPORTS) == name.startswith("exact_wide")
        getattr(libbang, fam.export)                                           # ... and the library exports it


def test_the_shape_table():
    assert S.SHAPES["one_workgroup"] == (1, None) and S.SHAPES["ragged"] == (3, 5) and S.SHAPES["full_chip"] == (None, None)
    assert S.caps("one_workgroup") == (1, 0) and S.caps("ragged") == (3, 5) and S.caps("full_chip") == (0, 0)
    # every narrow and wide input, in the three runs
    assert {c[1] for c in S.EXACT_CASES} == set(S.NARROW) | set(S.WIDE)
    assert {(c[2], c[3], c[4]) for c in S.EXACT_CASES} == {("one_workgroup", 37, 10), ("ragged", 37, 10), ("one_workgroup", 512, 512)}
    assert len(S.FULL_CASES) == 10 and len(S.EXACT_CASES) == 57
    with pytest.raises(AssertionError):
        S.assert_reached("one_workgroup", (S.NQ, 1), S.NQ, (256, 16))           # the default launch reaches nothing
    with pytest.raises(AssertionError):
        S.assert_reached("ragged", (3, 4), S.NQ, (256, 16))
    with pytest.raises(AssertionError):
        S.assert_reached("full_chip", (256, 8), 256 * 16 + 3, (256, 16))
