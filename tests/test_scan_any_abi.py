"""Option scan_any without a GPU: the exports and the option exist, bang_scan_any_geometry / bang_scan_any_check (csrc/bang_scan_host.cpp, no HIP call)
accept the any-dimension layouts and refuse the rest by name, and today's entries refuse what they refused."""
import ctypes as C

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
_GOOD = dict(d_vec_base=0x10000, vec_stride=100, dtype=1, D=100, n_nodes=4000, d_queries=0x20000, nq=64, k=10, stripes=2,
             d_scratch=0x30000, scratch_bytes=8 * 64 * 2 * 10 + 8 * 64, d_ids_out=0x40000, d_dists_out=0x50000, d_matched=0x60000)
# (changes to _GOOD, query elements or None = D) -> code, a word of the message
_CASES = [
    (dict(), None, OK, ""), (dict(), 99, OK, ""),                                                         # int8 D = 100, packed; its MIPS queries
    (dict(dtype=0, D=784, vec_stride=784 + 4 + 4 * 32), None, OK, ""), (dict(dtype=0, D=4, vec_stride=4), None, OK, ""),
    (dict(dtype=0, D=1024, vec_stride=1024), 1023, OK, ""), (dict(dtype=2, D=1, vec_stride=4), None, OK, ""),
    (dict(dtype=2, D=201, vec_stride=804), 200, OK, ""), (dict(dtype=2, D=1023, vec_stride=4092), None, OK, ""),
    (dict(dtype=0, D=128, vec_stride=128), None, OK, ""),                                                 # a narrow layout is served too
    (dict(D=18, vec_stride=20), None, ERR_UNSUPPORTED, "D % 4 == 0"), (dict(D=1028, vec_stride=1028), None, ERR_UNSUPPORTED, "D = 1028"),
    (dict(dtype=2, D=1028, vec_stride=4112), None, ERR_UNSUPPORTED, "D = 1028"), (dict(D=0), 0, ERR_UNSUPPORTED, "D = 0"),
    (dict(dtype=3), None, ERR_UNSUPPORTED, "dtype"), (dict(vec_stride=96), None, ERR_UNSUPPORTED, "vec_stride"),
    (dict(vec_stride=102), None, ERR_UNSUPPORTED, "vec_stride"), (dict(dtype=2, vec_stride=396), None, ERR_UNSUPPORTED, "vec_stride"),
    (dict(), 98, ERR_ARG, "qdim"), (dict(), 101, ERR_ARG, "qdim"), (dict(dtype=2, D=1, vec_stride=4), 0, ERR_ARG, "qdim"),
    (dict(k=129), None, ERR_ARG, "k = 129"), (dict(k=0), None, ERR_ARG, "k = 0"), (dict(nq=0), None, ERR_ARG, "nq = 0"),
    (dict(n_nodes=0), None, ERR_ARG, "n_nodes"), (dict(d_vec_base=0x10002), None, ERR_ARG, "d_vec_base"), (dict(d_queries=None), None, ERR_ARG, "d_queries"),
    (dict(d_labels=0x70000), None, ERR_ARG, "d_labels"), (dict(stripes=33), None, ERR_ARG, "stripes"), (dict(d_scratch=0x30004), None, ERR_ARG, "d_scratch"),
    (dict(scratch_bytes=8 * 64 * 2 * 10 + 8 * 64 - 1), None, ERR_ARG, "scratch_bytes"), (dict(d_ids_out=None), None, ERR_ARG, "d_ids_out"),
    (dict(d_dists_out=None), None, ERR_ARG, "d_dists_out"), (dict(d_matched=None), None, ERR_ARG, "d_matched"),
]


def _err(lib):
    lib.bang_last_error.restype = C.c_char_p
    return lib.bang_last_error().decode()


def test_exports_and_option(libbang):
    for sym in ("bang_k_scan_any", "bang_scan_any_check", "bang_scan_any_geometry"):
        getattr(libbang, sym)
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    assert "scan_any" in buf.value.decode() and "BANG_SCAN_ANY" in buf.value.decode()


@pytest.mark.parametrize("kw,qdim,code,word", _CASES)
def test_check_and_entry_before_any_hip_call(libbang, kw, qdim, code, word):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    from bang_amd import binding as B
    p = B.ScanParams()
    for k, v in {**_GOOD, **kw}.items():
        setattr(p, k, v)
    qdim = p.D if qdim is None else qdim
    libbang.bang_scan_any_check.argtypes = [C.c_void_p, C.c_uint32]
    libbang.bang_k_scan_any.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    assert libbang.bang_scan_any_check(C.byref(p), qdim) == code, (kw, _err(libbang))
    if code != OK:
        assert word in _err(libbang) and "bang_k_scan_any" in _err(libbang), (kw, _err(libbang))
        assert libbang.bang_k_scan_any(C.byref(p), qdim, None) == code and word in _err(libbang)


def test_geometry(libbang):
    lib = libbang
    for fn in (lib.bang_scan_any_geometry, lib.bang_scan_geometry):
        fn.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    t, s, t0, s0 = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    for dtype, D, qt in ((0, 784, 32), (1, 100, 32), (0, 4, 32), (2, 1, 16), (2, 201, 16), (2, 1023, 16)):
        for n, nq, k in ((1, 1, 1), (300, 8, 128), (1000000, 100, 10), (1000000, 4096, 100)):
            assert lib.bang_scan_any_geometry(dtype, D, nq, n, k, C.byref(t), C.byref(s)) == OK
            assert lib.bang_scan_geometry(dtype, 128, nq, n, k, C.byref(t0), C.byref(s0)) == OK       # the rule is the narrow layouts'
            assert (t.value, s.value) == (t0.value, s0.value) and t.value == -(-nq // qt)
    for dtype, D in ((0, 18), (0, 1028), (2, 1025), (2, 0), (3, 128)):
        assert lib.bang_scan_any_geometry(dtype, D, 1, 10, 1, C.byref(t), C.byref(s)) == ERR_UNSUPPORTED
    assert lib.bang_scan_any_geometry(0, 100, 0, 10, 1, C.byref(t), C.byref(s)) == ERR_ARG
    assert lib.bang_scan_any_geometry(0, 100, 1, 10, 129, C.byref(t), C.byref(s)) == ERR_ARG
    assert lib.bang_scan_geometry(0, 48, 1, 10, 1, C.byref(t), C.byref(s)) == ERR_UNSUPPORTED        # today's entry is what it was
