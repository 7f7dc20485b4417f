"""C-ABI of the beam form of the exact-distance search kernel (bang_k_search_exact_beam, csrc/bang_search_beam.hip), without a GPU: a broken
contract is refused with the right code and a message naming the member -- or `beam` -- BEFORE any HIP call (on a machine without a device a
launcher that reached the runtime would return BANG_ERR_HIP, not the code asserted here), and with the code and the text bang_k_search_exact
gives for the same arguments; bang_search_params is what it was."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
U8, I8, F32 = 0, 1, 2


def _params(B, **over):
    """Arguments of a pulled-rows launch that pass every check (the pointers are never dereferenced on the host)."""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter = 4, 32, 37, 0, 37 + 49
    sp.row_layout, sp.entry_len, sp.vec_bytes = 1, 256, 128
    sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = U8, 128, 10, 0, 4
    sp.rr_vec_stride = 128
    for f in ("d_seed", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query", "rr_queries", "rr_vec_base", "rr_ids_out", "rr_dists_out"):
        setattr(sp, f, 0x1000)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


def _call(libbang, sp, beam=2):
    f = libbang.bang_k_search_exact_beam
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    f.restype = C.c_int
    rc = f(C.byref(sp), beam, None)
    return rc, libbang.bang_last_error().decode()


def _same_as_the_exact_entry(libbang, B, over, rc, err, beam):
    """bang_k_search_exact on the same arguments: its code, and its message behind the prefix that names the beam"""
    f = libbang.bang_k_search_exact
    f.argtypes = [C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc_exact = f(C.byref(_params(B, **over)), None)
    err_exact = libbang.bang_last_error().decode()
    assert rc_exact != OK and err_exact.startswith("distance = 1"), (rc_exact, err_exact)
    assert rc == rc_exact, (rc, rc_exact, err)
    assert err == "distance = 1, beam = %d" % beam + err_exact[len("distance = 1"):], (err, err_exact)


@pytest.mark.parametrize("beam", [0, 5, 64, 0xFFFFFFFF])
def test_beam_out_of_range(libbang, beam):
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B), beam)
    assert rc == ERR_ARG and "beam" in err, (rc, err)
    rc, err = _call(libbang, _params(B, Q=0), beam)                    # (checked before the empty batch is waved through)
    assert rc == ERR_ARG and "beam" in err, (rc, err)


@pytest.mark.parametrize("over,message", [
    (dict(rr_vec_base=None), "rr_vec_base"),
    (dict(rr_vec_base=0x1002), "rr_vec_base"),
    (dict(rr_vec_stride=0), "rr_vec_stride"),
    (dict(rr_vec_stride=126), "rr_vec_stride"),                       # not divisible by 4
    (dict(rr_vec_stride=64), "rr_vec_stride"),                        # shorter than the vector
    (dict(rr_D=40, vec_bytes=40, rr_vec_stride=40), "rr_vec_stride"),  # 8-bit vectors with D % 16 != 0
    (dict(vec_bytes=0), "vec_bytes"),
    (dict(rr_dtype=F32, rr_D=32, vec_bytes=32), "vec_bytes"),
    (dict(n_slices=2), "d_row_slices"),
    (dict(n_slices=2, d_row_slices=0x1000), "slice_rows"),
    (dict(n_rows_hbm=5), "d_rows_hbm"),
    (dict(R=65), "R"),
    (dict(R=0), "R"),
    (dict(L=513), "L"),
    (dict(d_graph=None), "d_graph"),
    (dict(d_graph=0x1002), "d_graph"),
    (dict(d_bloom=None), "null buffer"),
    (dict(rr_ids_out=None), "null buffer"),
    (dict(cap_iter=0), "iteration cap"),
    (dict(cap_iter=37 + 50), "iteration cap"),
    (dict(rr_k=38), "k"),
    (dict(rr_Q_total=3), "result rows"),
    (dict(rr_vec_f16=2), "rr_vec_f16"),
])
def test_pulled_form_refuses_a_broken_contract(libbang, over, message):
    from bang_amd import binding as B
    for beam in (1, 4):
        rc, err = _call(libbang, _params(B, **over), beam)
        assert rc == ERR_ARG, (rc, err)
        assert message in err and "beam" in err, err
        _same_as_the_exact_entry(libbang, B, over, rc, err, beam)


@pytest.mark.parametrize("over", [
    dict(rr_vec_f16=1, rr_dtype=F32, rr_D=128, vec_bytes=512, rr_vec_stride=256),            # an fp16 vector table
    dict(rr_D=48, vec_bytes=48, rr_vec_stride=48),                                            # 8-bit, D / 16 = 3: a wide layout
    dict(rr_D=784, vec_bytes=784, rr_vec_stride=784),
    dict(rr_dtype=F32, rr_D=960, vec_bytes=3840, rr_vec_stride=3840),
    dict(row_layout=0, entry_len=48 + 4 * 33, rr_D=48, vec_bytes=48),                         # the same with graph entries in HBM
    dict(row_layout=0, entry_len=3840 + 4 * 33, rr_dtype=F32, rr_D=960, vec_bytes=3840),
])
def test_fp16_rows_and_wide_layouts_are_unsupported(libbang, over):
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, **over))
    assert rc == ERR_UNSUPPORTED and "beam" in err, (rc, err)


def test_row_layouts_and_the_graph_entry_form(libbang):
    from bang_amd import binding as B
    for layout in (2, 7):
        rc, err = _call(libbang, _params(B, row_layout=layout))
        assert rc == ERR_UNSUPPORTED and "row_layout" in err, (rc, err)
    rc, err = _call(libbang, _params(B, row_layout=0, d_graph=None, entry_len=128 + 4 * 33))
    assert rc == ERR_UNSUPPORTED and "d_graph" in err
    rc, err = _call(libbang, _params(B, row_layout=0, entry_len=130, rr_vec_base=None, rr_vec_stride=0))
    assert rc == ERR_UNSUPPORTED and "unsupported vector layout" in err
    rc, err = _call(libbang, _params(B, row_layout=0, entry_len=128 + 4 * 33, rr_queries=0x1001))
    assert rc == ERR_UNSUPPORTED and "unsupported vector layout" in err
    for over in (dict(row_layout=2), dict(row_layout=7), dict(row_layout=0, d_graph=None, entry_len=128 + 4 * 33),
                 dict(row_layout=0, entry_len=130, rr_vec_base=None, rr_vec_stride=0), dict(row_layout=0, entry_len=128 + 4 * 33, rr_queries=0x1001)):
        for beam in (1, 4):
            rc, err = _call(libbang, _params(B, **over), beam)
            _same_as_the_exact_entry(libbang, B, over, rc, err, beam)


def test_null_and_empty(libbang):
    from bang_amd import binding as B
    f = libbang.bang_k_search_exact_beam
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    assert f(None, 2, None) == ERR_ARG
    rc, _ = _call(libbang, _params(B, Q=0, rr_vec_base=None))           # an empty batch is no launch at all
    assert rc == OK


def test_layouts_the_beam_form_evaluates(libbang):
    f = libbang.bang_search_exact_beam_supported
    f.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    f.restype = C.c_int
    for dtype, D, stride in ((U8, 16, 16), (U8, 128, 388), (I8, 64, 64), (I8, 256, 256), (F32, 4, 16), (F32, 20, 80), (F32, 256, 1024), (F32, 96, 644)):
        assert f(dtype, D, stride) == 1, (dtype, D, stride)
    for dtype, D, stride in ((U8, 48, 48), (U8, 784, 784), (U8, 512, 512), (F32, 260, 1040), (F32, 960, 3840), (U8, 40, 40), (F32, 6, 24), (U8, 128, 126),
                             (F32, 128, 256), (3, 128, 128)):
        assert f(dtype, D, stride) == 0, (dtype, D, stride)


def test_geometry_refuses_before_any_device_call(libbang):
    for name in ("bang_search_exact_beam_geometry", "bang_search_exact_beam_pull_geometry"):
        g = getattr(libbang, name)
        g.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        g.restype = C.c_int
        wg, w = C.c_uint32(0), C.c_uint32(0)
        assert g(U8, 37, 0, 64, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG and "beam" in libbang.bang_last_error().decode()
        assert g(U8, 37, 5, 64, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG
        assert g(U8, 513, 2, 64, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG
        assert g(7, 37, 2, 64, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG
        assert g(U8, 37, 2, 0, 0, 0, C.byref(wg), C.byref(w)) == ERR_ARG
        assert g(U8, 37, 2, 64, 0, 0, None, C.byref(w)) == ERR_ARG


def test_header_declares_the_beam_entry_points(libbang):
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+bang_k_search_exact_beam\s*\(\s*const\s+bang_search_params\s*\*\s*\w*\s*,\s*uint32_t\s+beam\s*,\s*void\s*\*\s*\w*\s*\)", src)
    for name in ("bang_k_search_exact_beam", "bang_search_exact_beam_supported", "bang_search_exact_beam_geometry", "bang_search_exact_beam_pull_geometry"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert hasattr(libbang, name), name
    text = hdr[hdr.index("BEAM form of the exact-distance search kernel"):hdr.index("int bang_k_search_exact_beam(")]
    for word in ("beam", "filter state", "dropped", "cap_iter", "BANG_ERR_ARG", "BANG_ERR_UNSUPPORTED", "rr_vec_f16"):
        assert word in text, word
