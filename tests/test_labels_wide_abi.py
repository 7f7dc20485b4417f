"""C-ABI of label filters on the wide vector layouts (bang_k_search_exact_labels_wide, option labels_wide), without a GPU: export and option row
exist; the entry takes exactly the layouts bang_k_search_exact sends to the wide instances and refuses the rest by name BEFORE any HIP call."""
import ctypes as C

import pytest

OK, ERR_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NOGPU = 0, -1, -4, -5, -6
U8, I8, F32 = 0, 1, 2
P = 0x1000                       # a non-null "device pointer": never dereferenced on the host
WIDE = {"u8_48": (U8, 48, 48), "u8_192": (U8, 192, 192), "i8_1024": (I8, 1024, 1024), "f32_260": (F32, 260, 1040), "f32_1024": (F32, 1024, 4096)}


def _call(libbang, layout, dtype, D, vb, flt=(), **over):
    """Arguments that pass every check of bang_k_search_exact (graph entries in HBM: 0, pulled rows: 1), then `over`; filter members `flt` null"""
    from bang_amd import binding as B
    sp, lf = B.SearchParams(), B.LabelFilter()
    sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter, sp.n_nodes = 4, 32, 37, 0, 37 + 49, 4000
    sp.row_layout, sp.entry_len, sp.vec_bytes = layout, (256 if layout else vb + 4 * 33), vb
    sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total, sp.rr_vec_stride = dtype, D, 10, 0, 4, vb
    for f in ("d_seed", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query", "rr_queries", "rr_vec_base", "rr_ids_out", "rr_dists_out"):
        setattr(sp, f, P)
    for k, v in over.items():
        setattr(sp, k, v)
    lf.d_labels, lf.d_filters = (None if "d_labels" in flt else P), (None if "d_filters" in flt else P)
    f = libbang.bang_k_search_exact_labels_wide
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    return f(C.byref(sp), C.byref(lf), None), libbang.bang_last_error().decode()


def test_export_and_option_row(libbang):
    assert hasattr(libbang, "bang_k_search_exact_labels_wide")
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    buf = C.create_string_buffer(libbang.bang_describe_options(None, 0))
    libbang.bang_describe_options(buf, len(buf))
    row = [l for l in buf.value.decode().splitlines() if l.split()[:1] == ["labels_wide"]]
    assert len(row) == 1 and "BANG_LABELS_WIDE" in row[0] and "[0, 1]" in row[0] and "bang_alloc" in row[0], row


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_layouts_pass_every_host_check(libbang, name, layout):
    """A good launch gets as far as the runtime (without a device; with one, made-up pointers are not launched on: Q = 0 alone is asked)."""
    import bang_amd
    assert _call(libbang, layout, *WIDE[name], Q=0)[0] == OK
    if bang_amd.device_count() == 0:
        assert _call(libbang, layout, *WIDE[name])[0] in (ERR_HIP, ERR_NOGPU)
    for flt, over, word in ((("d_labels",), {}, "d_labels"), (("d_filters",), {}, "d_filters"), ((), dict(n_nodes=0), "n_nodes"), ((), dict(rr_k=38), "bad k")):
        rc, err = _call(libbang, layout, *WIDE[name], flt=flt, **over)
        assert rc == ERR_ARG and word in err, (rc, err)


@pytest.mark.parametrize("layout,over,word", [
    (0, dict(rr_D=128, vec_bytes=128, entry_len=128 + 4 * 33), "bang_k_search_exact_labels"),            # narrow 8-bit: the existing entry
    (1, dict(rr_dtype=F32, rr_D=256, vec_bytes=1024, rr_vec_stride=1024), "bang_k_search_exact_labels"),   # narrow float
    (1, dict(rr_vec_f16=1, rr_dtype=F32, rr_D=128, vec_bytes=512, rr_vec_stride=256), "rr_vec_f16"),
    (0, dict(any_dim=1, rr_D=100, vec_bytes=100, entry_len=100 + 4 * 33), "any_dim"),
    (1, dict(any_dim=1, rr_dtype=F32, rr_D=260, rr_qdim=259, vec_bytes=1040, rr_vec_stride=1040), "any_dim"),
])
def test_what_the_wide_label_instances_do_not_serve_is_refused_by_name(libbang, layout, over, word):
    rc, err = _call(libbang, layout, U8, 192, 192, **over)
    assert rc == ERR_UNSUPPORTED and word in err and "labels_wide" in err, (rc, err)
