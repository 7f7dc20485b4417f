"""C-ABI of the LUT-path search kernel, without a GPU: the header declares the three entries, bang_search_lut_supported agrees with the
per-wave LDS formula, and bang_k_search_lut refuses bad arguments with the right code and message BEFORE any HIP call (on a machine without a
device a launcher that reached the runtime would return BANG_ERR_HIP, not the code asserted here)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
LDS_BYTES = 160 * 1024


def _wave_bytes(L):
    """2L + L/4 (rounded up to 4 words) + 144 words: one wave's worklist and scratch."""
    return (((2 * L + (L + 3) // 4 + 3) & ~3) + 144) * 4


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    assert re.search(r"int\s+bang_k_search_lut\(const bang_search_params\*\s*p,\s*void\*\s*stream\);", hdr)
    assert re.search(r"int\s+bang_search_lut_supported\(uint32_t m,\s*uint32_t L\);", hdr)
    assert re.search(r"int\s+bang_search_lut_geometry\(uint32_t L,\s*uint32_t Q,\s*uint32_t max_wgs,\s*uint32_t max_waves,\s*uint32_t\*\s*workgroups,"
                     r"\s*uint32_t\*\s*waves\);", hdr)
    body = re.search(r"typedef struct \{(.*?)\}\s*bang_search_params\s*;", hdr, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", body, flags=re.S).strip().rstrip(";").split(";")
    assert re.search(r"const float\*\s*d_lut$", members[-1].strip())          # appended LAST: the earlier members keep their offsets


def test_supported_agrees_with_the_lds_formula(libbang):
    f = libbang.bang_search_lut_supported
    f.argtypes = [C.c_uint32, C.c_uint32]
    for L in (1, 512):
        assert _wave_bytes(L) <= LDS_BYTES
        for m in (1, 5, 65, 120, 1024):
            assert f(m, L) == 1
    assert _wave_bytes(512) == (1024 + 128 + 144) * 4
    for L in (0, 513, 1024, 1 << 20):
        assert f(64, L) == 0
    assert f(0, 64) == 0


def _params(B, **over):
    """Arguments that pass every check (the pointers are never dereferenced on the host)."""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.m, sp.L, sp.medoid, sp.cap_iter = 4, 32, 65, 37, 0, 37 + 49
    sp.entry_len, sp.vec_bytes = 4 * 65 + 4 * 33, 4 * 65
    for f in ("d_seed", "d_codes", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query", "d_lut"):
        setattr(sp, f, 0x1000)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


@pytest.mark.parametrize("over,code,message", [
    (dict(d_lut=None), ERR_ARG, "null buffer"),
    (dict(d_bloom=None), ERR_ARG, "null buffer"),
    (dict(d_seed=None), ERR_ARG, "null buffer"),
    (dict(d_cand_ids=None), ERR_ARG, "null buffer"),
    (dict(d_cand_cnt=None), ERR_ARG, "null buffer"),
    (dict(d_codes=None), ERR_ARG, "null buffer"),
    (dict(d_next_query=None), ERR_ARG, "null buffer"),
    (dict(psz=2, mp=68), ERR_UNSUPPORTED, "psz"),
    (dict(row_layout=1), ERR_UNSUPPORTED, "row_layout"),
    (dict(d_graph=None), ERR_UNSUPPORTED, "d_graph"),
    (dict(R=0), ERR_ARG, "bad R/L"),
    (dict(R=65), ERR_ARG, "bad R/L"),
    (dict(L=0), ERR_ARG, "bad R/L"),
    (dict(L=513, cap_iter=513 + 49), ERR_ARG, "bad R/L"),
    (dict(cap_iter=0), ERR_ARG, "iteration cap"),
    (dict(cap_iter=37 + 50), ERR_ARG, "iteration cap"),
    (dict(m=0), ERR_ARG, "code stride"),
    (dict(code_stride=64), ERR_ARG, "code stride"),
    (dict(entry_len=4 * 65 + 4 * 32), ERR_ARG, "graph entry"),
    (dict(d_codes=0x1001), ERR_ARG, "4-byte aligned"),
    (dict(d_lut=0x1002), ERR_ARG, "4-byte aligned"),
])
def test_launcher_refuses_bad_arguments(libbang, over, code, message):
    from bang_amd import binding as B
    f = libbang.bang_k_search_lut
    f.argtypes = [C.c_void_p, C.c_void_p]
    sp = _params(B, **over)
    assert f(C.byref(sp), None) == code
    assert message in libbang.bang_last_error().decode()


def test_launcher_null_and_empty(libbang):
    from bang_amd import binding as B
    f = libbang.bang_k_search_lut
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(None, None) == ERR_ARG
    sp = _params(B, Q=0, d_lut=None)                      # an empty batch is no launch at all
    assert f(C.byref(sp), None) == OK


def test_geometry_refuses_bad_arguments(libbang):
    g = libbang.bang_search_lut_geometry
    g.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
    wg, wv = C.c_uint32(), C.c_uint32()
    assert g(37, 0, 0, 0, C.byref(wg), C.byref(wv)) == ERR_ARG
    assert g(37, 4, 0, 0, None, C.byref(wv)) == ERR_ARG
    assert g(513, 4, 0, 0, C.byref(wg), C.byref(wv)) == ERR_ARG
