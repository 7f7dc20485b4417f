"""Option scan_mfma without a GPU: the exports and the option row, bang_scan_f32_mfma_check's refusals (csrc/bang_scan_mfma_host.cpp, no HIP call) on
made-up addresses, and the launch geometry."""
import ctypes as C

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
_GOOD = dict(d_vec_base=0x10000, vec_stride=296, dtype=2, D=74, n_nodes=4000, d_queries=0x20000, nq=64, k=10, stripes=2,
             d_scratch=0x30000, scratch_bytes=8 * 64 * 2 * 10 + 8 * 64, d_ids_out=0x40000, d_dists_out=0x50000, d_matched=0x60000)
# (changes to _GOOD, query elements or None = D) -> code, a word of the message
_CASES = [
    (dict(), None, OK, ""), (dict(), 73, OK, ""), (dict(D=1, vec_stride=4), None, OK, ""), (dict(D=1024, vec_stride=4096), 1023, OK, ""),
    (dict(stripes=32), None, ERR_ARG, "scratch_bytes"), (dict(stripes=33), None, ERR_ARG, "stripes"),       # 4000 points are 32 rounds of 128
    (dict(dtype=0), None, ERR_UNSUPPORTED, "not float"), (dict(dtype=1), None, ERR_UNSUPPORTED, "not float"),
    (dict(D=0), 0, ERR_UNSUPPORTED, "D = 0"), (dict(D=1025, vec_stride=4100), None, ERR_UNSUPPORTED, "D = 1025"),
    (dict(vec_stride=292), None, ERR_UNSUPPORTED, "vec_stride"), (dict(vec_stride=298), None, ERR_UNSUPPORTED, "vec_stride"),
    (dict(), 72, ERR_ARG, "qdim"), (dict(), 75, ERR_ARG, "qdim"), (dict(D=1, vec_stride=4), 0, ERR_ARG, "qdim"),
    (dict(k=129), None, ERR_ARG, "k = 129"), (dict(k=0), None, ERR_ARG, "k = 0"), (dict(nq=0), None, ERR_ARG, "nq = 0"),
    (dict(n_nodes=0), None, ERR_ARG, "n_nodes"), (dict(d_vec_base=0x10002), None, ERR_ARG, "d_vec_base"), (dict(d_queries=None), None, ERR_ARG, "d_queries"),
    (dict(d_labels=0x70000), None, ERR_ARG, "d_labels"), (dict(d_scratch=0x30004), None, ERR_ARG, "d_scratch"),
    (dict(d_ids_out=None), None, ERR_ARG, "d_ids_out"), (dict(d_dists_out=None), None, ERR_ARG, "d_dists_out"), (dict(d_matched=None), None, ERR_ARG, "d_matched"),
]


def _err(lib):
    lib.bang_last_error.restype = C.c_char_p
    return lib.bang_last_error().decode()


def test_exports_and_option_row(libbang):
    for sym in ("bang_k_scan_f32_mfma", "bang_scan_f32_mfma_check", "bang_scan_f32_mfma_geometry", "bang_scan_f32_mfma_max_stripes", "bang_get_scan_counters_e"):
        getattr(libbang, sym)
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    row = [ln for ln in buf.value.decode().splitlines() if ln.split()[:1] == ["scan_mfma"]]
    assert len(row) == 1 and row[0].split()[1:5] == ["BANG_SCAN_MFMA", "[0,", "1]", "any"], row


@pytest.mark.parametrize("kw,qdim,code,word", _CASES)
def test_check_and_entry_before_any_hip_call(libbang, kw, qdim, code, word):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    from bang_amd import binding as B
    p = B.ScanParams()
    for k, v in {**_GOOD, **kw}.items():
        setattr(p, k, v)
    before = bytes(p)
    qdim = p.D if qdim is None else qdim
    libbang.bang_scan_f32_mfma_check.argtypes = [C.c_void_p, C.c_uint32]
    libbang.bang_k_scan_f32_mfma.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    assert libbang.bang_scan_f32_mfma_check(C.byref(p), qdim) == code, (kw, _err(libbang))
    if code != OK:
        assert word in _err(libbang) and "bang_k_scan_f32_mfma" in _err(libbang), (kw, _err(libbang))
        assert libbang.bang_k_scan_f32_mfma(C.byref(p), qdim, None, None) == code and word in _err(libbang)
    assert bytes(p) == before


def test_geometry(libbang):
    lib = libbang
    lib.bang_scan_f32_mfma_geometry.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
    t, s = C.c_uint32(0), C.c_uint32(0)
    for D in (1, 74, 1024):
        for n, nq, k in ((1, 1, 1), (129, 1, 1), (300, 8, 128), (1000000, 100, 10), (1000000, 4096, 100), (1000000, 1, 128)):
            assert lib.bang_scan_f32_mfma_geometry(D, nq, n, k, C.byref(t), C.byref(s)) == OK
            per = -(-(-(-n // s.value)) // 128) * 128            # points of a stripe, as the launch rounds them
            assert t.value == -(-nq // 32) and 1 <= s.value == min(s.value, lib.bang_scan_f32_mfma_max_stripes(n, k))
            assert s.value * k <= 4096 and (s.value - 1) * per < n, (D, n, nq, k, s.value)
    assert lib.bang_scan_f32_mfma_max_stripes(4000, 10) == 32 and lib.bang_scan_f32_mfma_max_stripes(1000000, 128) == 32
    for D in (0, 1025):
        assert lib.bang_scan_f32_mfma_geometry(D, 1, 10, 1, C.byref(t), C.byref(s)) == ERR_UNSUPPORTED
    assert lib.bang_scan_f32_mfma_geometry(74, 0, 10, 1, C.byref(t), C.byref(s)) == ERR_ARG
    assert lib.bang_scan_f32_mfma_geometry(74, 1, 10, 129, C.byref(t), C.byref(s)) == ERR_ARG
