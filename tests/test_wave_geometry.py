"""bang_wave_geometry (csrc/bang_wave_host.cpp): the launch geometry the exact-distance, beam and LUT search kernels share, without a GPU.  The
public *_geometry functions read a kernel's register count and launch bound off the device and hand them to this function, which is arithmetic
alone: known answers worked out by hand from the rule, then a sweep against a restatement of the rule."""
import ctypes as C
import itertools
import os

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
CUS = 256


def wl_words(L):
    return (2 * L + (L + 3) // 4 + 3) & ~3


def plain_bytes(L):
    return 4 * (wl_words(L) + 144)


def labels_bytes(L):
    return 4 * (2 * wl_words(L) + 144)


def beam_bytes(L, beam):
    return 4 * (wl_words(L) + 144 + 2 * (64 * beam + 4))


def geometry(libbang, regs, max_waves_wg, wave_bytes, Q, max_wgs=0, max_waves=0, cus=CUS):
    f = libbang.bang_wave_geometry
    f.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)] * 2
    f.restype = C.c_int
    wg, w = C.c_uint32(0xDEAD), C.c_uint32(0xDEAD)
    rc = f(regs, max_waves_wg, wave_bytes, cus, Q, max_wgs, max_waves, C.byref(wg), C.byref(w))
    return (rc, wg.value, w.value) if rc == OK else (rc, None, None)


def restated(regs, max_waves_wg, wave_bytes, cus, Q, max_wgs, max_waves):
    """Registers in granules of 8 out of 512 per SIMD lane, at most 8 waves per SIMD, four SIMDs; 160 KB of LDS; at most 32 waves per CU; one
    workgroup of at most 16 waves within the launch bound; a small batch on all CUs with fewer waves each."""
    per_cu = min(4 * min(512 // (-(-regs // 8) * 8), 8), 160 * 1024 // wave_bytes, 32)
    if per_cu == 0:
        return ERR_UNSUPPORTED, None, None
    full = min(per_cu, 16, max_waves_wg)
    W = min(full, max_waves) if max_waves else full
    if Q <= cus * W:
        grid = min(Q, cus, max_wgs) if max_wgs else min(Q, cus)
        return OK, grid, min(W, -(-Q // grid))
    grid = min(cus * (per_cu // full), -(-Q // W))
    return OK, (min(grid, max_wgs) if max_wgs else grid), W


def test_known_answers(libbang):
    assert plain_bytes(152) == 1952 and labels_bytes(512) == 9792
    # the narrow instances: 98 VGPRs -> 104 allocated, 4 waves per SIMD, 16 per CU
    assert geometry(libbang, 98, 16, 1952, 10000) == (OK, 256, 16)
    assert geometry(libbang, 98, 16, 1952, 1000) == (OK, 256, 4)       # fewer than 16 queries per CU: all CUs, ceil(1000 / 256) waves each
    assert geometry(libbang, 98, 16, 1952, 100) == (OK, 100, 1)
    # the wide float pulled instance: 134 VGPRs -> 136 allocated, 3 waves per SIMD, 12 per CU (its launch bound)
    assert geometry(libbang, 134, 12, 1952, 10000) == (OK, 256, 12)
    # label filters at L = 512: 163 840 / 9 792 = 16 waves still fit LDS
    assert geometry(libbang, 118, 16, 9792, 10000) == (OK, 256, 16)
    # ... and at twice that per wave LDS is the bound: 8 waves per CU
    assert geometry(libbang, 118, 16, 2 * 9792, 10000) == (OK, 256, 8)
    # few registers and little LDS: 32 waves per CU are two workgroups of 16
    assert geometry(libbang, 64, 16, 1952, 100000) == (OK, 512, 16)


def test_one_wave_that_does_not_fit_is_unsupported(libbang):
    assert geometry(libbang, 98, 16, 163840, 100)[0] == OK
    assert geometry(libbang, 98, 16, 163841, 100)[0] == ERR_UNSUPPORTED
    assert geometry(libbang, 98, 16, 1 << 20, 100)[0] == ERR_UNSUPPORTED


def test_caps_are_honoured_in_both_branches(libbang):
    # a batch that fills the device
    assert geometry(libbang, 98, 16, 1952, 10000, max_wgs=40) == (OK, 40, 16)
    assert geometry(libbang, 98, 16, 1952, 10000, max_waves=4) == (OK, 256, 4)
    assert geometry(libbang, 98, 16, 1952, 10000, max_wgs=40, max_waves=4) == (OK, 40, 4)
    assert geometry(libbang, 98, 16, 1952, 10000, max_wgs=1000, max_waves=64) == (OK, 256, 16)     # caps above the geometry change nothing
    # a small batch spread over the CUs
    assert geometry(libbang, 98, 16, 1952, 1000, max_wgs=40) == (OK, 40, 16)                        # 25 queries per workgroup: 16 waves
    assert geometry(libbang, 98, 16, 1952, 1000, max_waves=2) == (OK, 256, 2)
    assert geometry(libbang, 98, 16, 1952, 100, max_wgs=40, max_waves=2) == (OK, 40, 2)
    assert geometry(libbang, 98, 16, 1952, 100, max_wgs=1000, max_waves=64) == (OK, 100, 1)


def test_bad_arguments(libbang):
    f = libbang.bang_wave_geometry
    f.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)] * 2
    f.restype = C.c_int
    wg, w = C.c_uint32(0), C.c_uint32(0)
    assert f(98, 16, 1952, CUS, 0, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG
    assert f(98, 16, 1952, CUS, 100, 0, 0, None, C.byref(w)) == ERR_ARG
    assert f(98, 16, 1952, CUS, 100, 0, 0, C.byref(wg), None) == ERR_ARG
    for regs, bound, nbytes, cus in ((0, 16, 1952, CUS), (98, 0, 1952, CUS), (98, 16, 0, CUS), (98, 16, 1952, 0)):    # nothing to divide by
        assert f(regs, bound, nbytes, cus, 100, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG


def test_the_walk_stages_are_written_once():
    """The stages the exact, beam and LUT kernels share live in csrc/bang_wave_walk.h (the hand-out counter, the filter with its atomic ORs, the
    parent rule) and the launch in wave_kernel_launch (bang_device.h): none of the three sources carries a copy of its own.  The beam's
    four-row filter is a different algorithm and keeps its ORs."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bang-billion-scale-ann_amd", "csrc")
    sources = ("bang_search_exact.hip", "bang_search_beam.hip", "bang_search_lut.hip")
    text = {f: open(os.path.join(csrc, f)).read() for f in sources + ("bang_wave_walk.h",)}
    for f in sources:
        for copy in ("__hip_atomic_fetch_add(p.d_next_query", "wave_min_key(", "hipFuncAttributeMaxDynamicSharedMemorySize"):
            assert copy not in text[f], (f, copy)
        assert '#include "bang_wave_walk.h"' in text[f], f
    assert sorted(f for f in text if "__hip_atomic_fetch_or" in text[f]) == ["bang_search_beam.hip", "bang_wave_walk.h"]


def test_the_search_kernels_host_side_and_layout_list_are_written_once():
    """csrc/bang_search.hip holds the kernel and its instance dispatch; the argument checks, the geometry and the entry points live in
    csrc/bang_search_host.cpp.  The compiled PQ layouts are listed once, in csrc/bang_search_args.h: no source switches over hand-written keys."""
    import glob
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bang-billion-scale-ann_amd", "csrc")
    text = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(csrc, "*"))}
    kernel = text["bang_search.hip"]
    assert "getenv(" not in kernel and "bang_k_search" not in kernel and not re.search(r"\bint bang_search_geometry\(", kernel)
    assert '#include "bang_search_args.h"' in kernel and "BANG_SEARCH_LAYOUTS(" in kernel
    keys = "|".join(str(100 * psz + ndw) for psz, ndw in ((1, 8), (1, 16), (1, 24), (1, 32), (2, 8), (2, 16), (2, 18), (2, 19), (4, 4), (4, 8), (8, 2), (8, 4)))
    for name, body in text.items():
        if name.endswith(".hip"):
            assert not re.search(rf"\bcase\s+({keys})\s*:", body), name
        assert "kNdwList" not in body, name
    assert sorted(name for name, body in text.items() if re.search(r"#define BANG_PQ_LAYOUTS\(", body)) == ["bang_search_args.h"]


@pytest.mark.parametrize("regs", [64, 97, 104, 105, 128, 134, 256])
def test_sweep_against_the_restated_rule(libbang, regs):
    sizes = [f(L) for L in (1, 37, 152, 512) for f in (plain_bytes, labels_bytes, *(lambda L, b=b: beam_bytes(L, b) for b in (2, 3, 4)))]
    for bound, nbytes, Q, (max_wgs, max_waves) in itertools.product((12, 16), sizes, (1, 255, 256, 257, 4096, 4097, 100000),
                                                                    ((0, 0), (7, 0), (0, 3), (300, 13))):
        got = geometry(libbang, regs, bound, nbytes, Q, max_wgs, max_waves)
        assert got == restated(regs, bound, nbytes, CUS, Q, max_wgs, max_waves), (regs, bound, nbytes, Q, max_wgs, max_waves)
        if got[0] == OK:                                                       # a launch is never empty, a workgroup never past its bound
            assert 1 <= got[2] <= bound and got[1] >= 1
