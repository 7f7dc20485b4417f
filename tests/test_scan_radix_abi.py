"""Option scan_radix without a GPU: the exports and the option row exist, bang_scan_radix_check / bang_k_scan_radix (csrc/bang_scan_radix_host.cpp, no
HIP call) accept k up to 4096 on the range scan's layouts with queries of D or D - 1 elements and refuse the rest with the member named, and the
geometry keeps its invariants."""
import ctypes as C

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
NQ, N = 64, 4000                                                            # max_runs = ceil(4000 / 32) = 125


def _scratch(nq, k):
    return 8 * nq + 4 * 256 * nq + 20 * nq + 8 * nq * k + 8                  # the layout bang_c.h documents


_GOOD = dict(d_vec_base=0x10000, vec_stride=100, dtype=1, D=100, n_nodes=N, d_queries=0x20000, nq=NQ, k=1000, stripes=2,
             d_scratch=0x30000, scratch_bytes=_scratch(NQ, 1000), d_ids_out=0x40000, d_dists_out=0x50000, d_matched=0x60000)
# (changes to _GOOD, query elements or None = D) -> code, a word of the message
_CASES = [(dict(k=k, scratch_bytes=_scratch(NQ, k)), qdim, OK, "") for k in (1, 129, 4096) for qdim in (None, 99)] + [
    (dict(dtype=0, D=1024, vec_stride=1024), 1023, OK, ""), (dict(dtype=2, D=1, vec_stride=4), None, OK, ""), (dict(dtype=2, D=201, vec_stride=804), 200, OK, ""),
    (dict(stripes=125), None, OK, ""), (dict(stripes=0), None, OK, ""),
    (dict(k=0), None, ERR_ARG, "k = 0"), (dict(k=4097, scratch_bytes=_scratch(NQ, 4097)), None, ERR_ARG, "k = 4097"),
    (dict(), 98, ERR_ARG, "qdim"), (dict(), 101, ERR_ARG, "qdim"),
    (dict(D=0), 0, ERR_UNSUPPORTED, "D = 0"), (dict(dtype=2, D=1025, vec_stride=4100), None, ERR_UNSUPPORTED, "D = 1025"),
    (dict(D=6, vec_stride=8), None, ERR_UNSUPPORTED, "D % 4 == 0"), (dict(dtype=3), None, ERR_UNSUPPORTED, "dtype"),
    (dict(d_vec_base=0x10002), None, ERR_ARG, "d_vec_base"), (dict(d_queries=0x20001), None, ERR_ARG, "d_queries"),
    (dict(vec_stride=96), None, ERR_UNSUPPORTED, "vec_stride"), (dict(vec_stride=102), None, ERR_UNSUPPORTED, "vec_stride"),
    (dict(scratch_bytes=_scratch(NQ, 1000) - 1), None, ERR_ARG, "scratch_bytes"), (dict(d_scratch=0x30004), None, ERR_ARG, "d_scratch"),
    (dict(stripes=126), None, ERR_ARG, "stripes"), (dict(d_labels=0x70000), None, ERR_ARG, "d_labels"),
    (dict(d_ids_out=None), None, ERR_ARG, "d_ids_out"), (dict(d_dists_out=None), None, ERR_ARG, "d_dists_out"), (dict(d_matched=None), None, ERR_ARG, "d_matched"),
]


def _err(lib):
    lib.bang_last_error.restype = C.c_char_p
    return lib.bang_last_error().decode()


def test_exports_and_option_row(libbang):
    for sym in ("bang_k_scan_radix", "bang_scan_radix_check", "bang_scan_radix_geometry", "bang_scan_radix_scratch_bytes"):
        getattr(libbang, sym)
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    row = [ln for ln in buf.value.decode().splitlines() if ln.startswith("  scan_radix ")]
    assert len(row) == 1 and "BANG_SCAN_RADIX" in row[0] and "[0, 2]" in row[0] and "any time" in row[0], row


@pytest.mark.parametrize("kw,qdim,code,word", _CASES)
def test_check_and_entry_before_any_hip_call(libbang, kw, qdim, code, word):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    from bang_amd import binding as B
    p = B.ScanParams()
    for k, v in {**_GOOD, **kw}.items():
        setattr(p, k, v)
    qdim = p.D if qdim is None else qdim
    libbang.bang_scan_radix_check.argtypes = [C.c_void_p, C.c_uint32]
    libbang.bang_k_scan_radix.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    assert libbang.bang_scan_radix_check(C.byref(p), qdim) == code, (kw, _err(libbang))
    if code != OK:
        assert word in _err(libbang) and "bang_k_scan_radix" in _err(libbang), (kw, _err(libbang))
        assert libbang.bang_k_scan_radix(C.byref(p), qdim, None) == code and word in _err(libbang)


def test_geometry_and_scratch(libbang):
    lib = libbang
    lib.bang_scan_radix_geometry.argtypes = [C.c_int] + [C.c_uint32] * 4 + [C.c_void_p] * 3
    lib.bang_scan_radix_scratch_bytes.argtypes, lib.bang_scan_radix_scratch_bytes.restype = [C.c_uint32] * 3, C.c_uint64
    t, r, most = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    for dtype, D, qt in ((0, 128, 32), (1, 100, 32), (2, 1, 16), (2, 1023, 16)):
        for n in (1, 31, 33, 4101, 1000000, (1 << 32) - 1):
            for nq, k in ((1, 1), (33, 4096), (4096, 1000), (1 << 20, 129)):
                assert lib.bang_scan_radix_geometry(dtype, D, nq, n, k, C.byref(t), C.byref(r), C.byref(most)) == OK
                tiles32 = -(-n // 32)
                per = -(-tiles32 // r.value) * 32                            # the points of a run, as the entry cuts them: whole 32-point tiles
                assert t.value == -(-nq // qt) and 1 <= r.value <= most.value <= min(tiles32, 4096) and per % 32 == 0 and per * r.value >= n
    sizes = [lib.bang_scan_radix_scratch_bytes(nq, k, runs) for nq in (1, 33, 4096) for k in (1, 129, 4096) for runs in (1, 4096)]
    assert sizes[0] == _scratch(1, 1) and sizes[-1] == _scratch(4096, 4096)
    assert all(lib.bang_scan_radix_scratch_bytes(nq + 1, k, 1) > lib.bang_scan_radix_scratch_bytes(nq, k, 1) and
               lib.bang_scan_radix_scratch_bytes(nq, k + 1, 1) > lib.bang_scan_radix_scratch_bytes(nq, k, 1) and
               lib.bang_scan_radix_scratch_bytes(nq, k, 9) >= lib.bang_scan_radix_scratch_bytes(nq, k, 1) for nq in (1, 33) for k in (1, 4095))
    for dtype, D in ((0, 6), (2, 1025), (2, 0), (3, 128)):
        assert lib.bang_scan_radix_geometry(dtype, D, 1, 10, 1, C.byref(t), C.byref(r), None) == ERR_UNSUPPORTED
    assert lib.bang_scan_radix_geometry(0, 100, 1, 10, 4097, C.byref(t), C.byref(r), None) == ERR_ARG
    assert lib.bang_scan_radix_geometry(0, 100, 1, 10, 4096, C.byref(t), C.byref(r), None) == OK        # max_runs may be NULL
