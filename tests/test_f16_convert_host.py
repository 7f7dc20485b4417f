"""csrc/bang_f16.h on the CPU: the integer routine behind bang_k_f32_to_f16 (option vectors_fp16) is plain C, so the same text is compiled for the
host here and compared with numpy's float32 -> float16 conversion (round to nearest even, subnormals, NaN payload rule) bit for bit: every
251st of the 2^32 float bit patterns, every pattern within 4096 of the boundaries of the routine's cases, and the overflow flag (a FINITE
value that becomes inf)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "bang_f16.h"
extern "C" void convert(const uint32_t* x, uint16_t* h, uint8_t* over, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) { bool o; h[i] = (uint16_t)f32_to_f16_bits(x[i], &o); over[i] = o ? 1 : 0; }
}
'''


@pytest.fixture(scope="module")
def convert(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("f16")
    (d / "c.cpp").write_text(SRC)
    so = str(d / "libc16.so")
    subprocess.check_call([cxx, "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc"), "-o", so, str(d / "c.cpp")])
    lib = C.CDLL(so)
    lib.convert.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]

    def run(bits: np.ndarray):
        bits = np.ascontiguousarray(bits, np.uint32)
        h, o = np.empty(bits.size, np.uint16), np.empty(bits.size, np.uint8)
        lib.convert(bits.ctypes.data, h.ctypes.data, o.ctypes.data, bits.size)
        return h, o
    return run


def _check(convert, bits):
    got, over = convert(bits)
    f = bits.view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        want = f.astype(np.float16).view(np.uint16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:4]]
    want_over = np.isfinite(f) & ((want & 0x7FFF) == 0x7C00)
    assert np.array_equal(over.astype(bool), want_over)


def test_strided_sweep_of_all_bit_patterns(convert):
    for start in range(0, 1 << 32, 1 << 28):                       # 16 slices of 2^28 / 251 patterns
        _check(convert, np.arange(start, start + (1 << 28), 251, dtype=np.uint64).astype(np.uint32))


def test_every_pattern_around_the_case_boundaries(convert):
    # zero | 2^-25 (tie with 0) | 2^-24 | 2^-14 (first normal half) | 1 + 2^-11 (a tie) | 65504 | 65520 (first inf) | inf | the first NaNs | the last
    for edge in (0x00000000, 0x33000000, 0x33800000, 0x38800000, 0x3F801000, 0x477FE000, 0x477FF000, 0x7F800000, 0x7F802000, 0x7FFFF000):
        lo = max(edge - 4096, 0)
        bits = np.arange(lo, min(edge + 4096, 0x7FFFFFFF) + 1, dtype=np.uint64).astype(np.uint32)
        _check(convert, bits)
        _check(convert, bits | np.uint32(0x80000000))
