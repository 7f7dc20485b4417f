"""C-ABI of per-query label filters (bang_k_search_exact_labels, bang_set_labels_e / bang_set_query_filters_e, bang_stats_ext3), without a GPU: the
symbols are exported and documented, a broken contract is refused with its code and a message naming the member BEFORE any HIP call (on a machine
without a device a launcher that reached the runtime would return BANG_ERR_HIP), header and ctypes mirrors agree on the new structs and
bang_search_params is what it was, and the two new code objects hold one instance per vector type, without scratch, in at most 128 VGPRs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
U8, I8, F32 = 0, 1, 2
P = 0x1000                       # a non-null "device pointer": never dereferenced on the host
SEARCH_PARAMS_SIZE, D_LUT_OFFSET = 376, 368     # bang_search_params before this entry point existed: d_lut its last member (tests/test_vectors_fp16_abi.py)


def _params(B, layout=0, **over):
    """Arguments that pass every check of bang_k_search_exact: graph entries in HBM (0) or pulled rows (1), the SIFT-like narrow layout"""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter, sp.n_nodes = 4, 32, 37, 0, 37 + 49, 4000
    sp.row_layout, sp.entry_len, sp.vec_bytes = layout, (256 if layout else 128 + 4 * 33), 128
    sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = U8, 128, 10, 0, 4
    sp.rr_vec_stride = 128
    for f in ("d_seed", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query", "rr_queries", "rr_vec_base", "rr_ids_out", "rr_dists_out"):
        setattr(sp, f, P)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


def _filter(B, **over):
    f = B.LabelFilter()
    f.d_labels, f.d_filters, f.d_excluded, f.d_matched = P, P, None, None
    for k, v in over.items():
        setattr(f, k, v)
    return f


def _call(libbang, sp, lf):
    f = libbang.bang_k_search_exact_labels
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(C.byref(sp) if sp is not None else None, C.byref(lf) if lf is not None else None, None)
    return rc, libbang.bang_last_error().decode()


def test_symbols_are_exported(libbang):
    for name in ("bang_k_search_exact_labels", "bang_search_exact_labels_geometry", "bang_search_exact_labels_pull_geometry", "bang_set_labels_e",
                 "bang_clear_labels_e", "bang_set_query_filters_e", "bang_clear_query_filters_e", "bang_get_matched_counts", "bang_get_stats_ext3"):
        assert hasattr(libbang, name), name


@pytest.mark.parametrize("layout", (0, 1))
def test_filter_arguments_are_refused_with_the_member_named(libbang, layout):
    from bang_amd import binding as B
    assert _call(libbang, None, _filter(B))[0] == ERR_ARG
    for empty in (dict(), dict(Q=0)):                                  # (checked before an empty batch is waved through)
        rc, err = _call(libbang, _params(B, layout, **empty), None)
        assert rc == ERR_ARG and "bang_label_filter" in err, (rc, err)
        for member in ("d_labels", "d_filters"):
            rc, err = _call(libbang, _params(B, layout, **empty), _filter(B, **{member: None}))
            assert rc == ERR_ARG and member in err, (rc, err)
        rc, err = _call(libbang, _params(B, layout, n_nodes=0, **empty), _filter(B))
        assert rc == ERR_ARG and "n_nodes" in err, (rc, err)
    assert _call(libbang, _params(B, layout, Q=0), _filter(B))[0] == OK  # an empty batch is no launch at all


@pytest.mark.parametrize("layout,over,code,message", [
    (0, dict(R=65), ERR_ARG, "bad R/L"),
    (0, dict(L=0), ERR_ARG, "bad R/L"),
    (0, dict(d_graph=None), ERR_UNSUPPORTED, "d_graph"),
    (0, dict(d_bloom=None), ERR_ARG, "null buffer"),
    (0, dict(cap_iter=0), ERR_ARG, "iteration cap"),
    (0, dict(rr_k=38), ERR_ARG, "bad k"),
    (0, dict(rr_Q_total=3), ERR_ARG, "result rows"),
    (0, dict(entry_len=130), ERR_UNSUPPORTED, "unsupported vector layout"),
    (0, dict(row_layout=2), ERR_UNSUPPORTED, "row_layout"),
    (0, dict(rr_vec_f16=2), ERR_ARG, "rr_vec_f16"),
    (1, dict(rr_vec_base=None), ERR_ARG, "rr_vec_base"),
    (1, dict(rr_vec_stride=126), ERR_ARG, "rr_vec_stride"),
    (1, dict(vec_bytes=0), ERR_ARG, "vec_bytes"),
    (1, dict(n_slices=2), ERR_ARG, "d_row_slices"),
    (1, dict(n_rows_hbm=5), ERR_ARG, "d_rows_hbm"),
    (1, dict(R=65), ERR_ARG, "R"),
    (1, dict(d_graph=0x1002), ERR_ARG, "d_graph"),
])
def test_every_check_of_the_unfiltered_entry_is_made(libbang, layout, over, code, message):
    """The code and message bang_k_search_exact gives for the same arguments."""
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, layout, **over), _filter(B))
    assert rc == code and message in err, (rc, err)
    f = libbang.bang_k_search_exact
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(C.byref(_params(B, layout, **over)), None) == code and libbang.bang_last_error().decode() == err


@pytest.mark.parametrize("layout,over,message", [
    (1, dict(rr_vec_f16=1, rr_dtype=F32, rr_D=128, vec_bytes=512, rr_vec_stride=256), "rr_vec_f16"),
    (0, dict(rr_D=48, vec_bytes=48, entry_len=48 + 4 * 33), "wide"),          # 8-bit, D / 16 = 3: a wide instance
    (1, dict(rr_D=48, vec_bytes=48, rr_vec_stride=48), "wide"),
    (0, dict(rr_dtype=F32, rr_D=512, vec_bytes=2048, entry_len=2048 + 4 * 33), "wide"),
])
def test_fp16_rows_and_wide_layouts_are_unsupported(libbang, layout, over, message):
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, layout, **over), _filter(B))
    assert rc == ERR_UNSUPPORTED and message in err and "labels" in err, (rc, err)


def test_engine_calls_are_refused_without_index_or_allocation(libbang):
    """Every engine entry is refused, with a message, before any device call."""
    h = C.c_void_p()
    assert libbang.bang_create(0, C.byref(h)) == 0
    setl = libbang.bang_set_labels_e
    setl.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    clrl = libbang.bang_clear_labels_e
    clrl.argtypes = [C.c_void_p]
    setf = libbang.bang_set_query_filters_e
    setf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    clrf = libbang.bang_clear_query_filters_e
    clrf.argtypes = [C.c_void_p]
    getm = libbang.bang_get_matched_counts
    getm.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    w = np.array([1, 2, 3], np.uint32)
    wp = w.ctypes.data_as(C.c_void_p)
    assert setl(h, wp, 3) == ERR_ARG and "no index is loaded" in libbang.bang_last_error().decode()
    assert clrl(h) == ERR_ARG and "no index is loaded" in libbang.bang_last_error().decode()
    assert setf(h, wp, wp, 3) == ERR_ARG and "bang_alloc" in libbang.bang_last_error().decode()
    assert clrf(h) == OK                                               # nothing to drop
    assert getm(h, wp, 3) == ERR_ARG and "filters" in libbang.bang_last_error().decode()
    assert setl(None, None, 0) == ERR_ARG and clrl(None) == ERR_ARG and setf(None, None, None, 0) == ERR_ARG and clrf(None) == ERR_ARG
    assert getm(None, None, 0) == ERR_ARG and libbang.bang_get_stats_ext3(None, None) == ERR_ARG
    libbang.bang_destroy.argtypes = [C.c_void_p]
    libbang.bang_destroy(h)


def test_a_bad_filter_file_is_refused_before_any_device_call(libbang, tmp_path, monkeypatch):
    """BANG_QUERY_FILTER_FILE, read by the bang.h bang_query through a helper that is not part of include/bang_c.h: unset is no filter at all; a
    missing file, a file of another layout, a header that promises more rows than the file holds and a file with fewer rows than the batch has
    queries are errors that name the variable and the file."""
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    assert "bang_apply_query_filter_file_e" not in hdr
    h = C.c_void_p()
    assert libbang.bang_create(0, C.byref(h)) == 0
    apply = libbang.bang_apply_query_filter_file_e
    apply.argtypes = [C.c_void_p, C.c_int]
    monkeypatch.delenv("BANG_QUERY_FILTER_FILE", raising=False)
    assert apply(h, 4) == OK
    odd, few = tmp_path / "odd.bin", tmp_path / "few.bin"
    odd.write_bytes(np.array([3, 1], np.int32).tobytes() + bytes(12))              # one column
    few.write_bytes(np.array([3, 2], np.int32).tobytes() + bytes(24))
    huge = tmp_path / "huge.bin"
    huge.write_bytes(np.array([0x7FFFFFFF, 2], np.int32).tobytes() + bytes(24))
    for path, word in ((tmp_path / "missing.bin", "cannot be opened"), (odd, "not a .bin file"), (huge, "not a .bin file"), (few, "the batch has 4 queries")):
        monkeypatch.setenv("BANG_QUERY_FILTER_FILE", str(path))
        assert apply(h, 4) != OK
        err = libbang.bang_last_error().decode()
        assert word in err and "BANG_QUERY_FILTER_FILE" in err and str(path) in err, err
    monkeypatch.setenv("BANG_QUERY_FILTER_FILE", str(few))
    assert apply(h, 3) == ERR_ARG and "bang_alloc" in libbang.bang_last_error().decode()     # a good file: on to bang_set_query_filters_e
    libbang.bang_destroy.argtypes = [C.c_void_p]
    libbang.bang_destroy(h)


def test_python_binding(libbang):
    import bang_amd
    for name in ("set_labels", "clear_labels", "set_filters", "clear_filters", "matched_counts"):
        assert callable(getattr(bang_amd.Engine, name)), name
    e = bang_amd.Engine("uint8")
    try:
        with pytest.raises(bang_amd.BangError, match="out of range"):
            e.set_labels([3, -1])
        with pytest.raises(bang_amd.BangError, match="out of range"):
            e.set_labels(np.array([1 << 32], np.int64))
        with pytest.raises(bang_amd.BangError, match="integers"):
            e.set_labels([0.5])
        with pytest.raises(bang_amd.BangError, match="no index is loaded"):
            e.set_labels(np.array([5], np.int16))
        with pytest.raises(bang_amd.BangError, match="`all`"):
            e.set_filters([1, 2], [1])
        with pytest.raises(bang_amd.BangError, match="`any` is out of range"):
            e.set_filters([-1], [0])
        with pytest.raises(bang_amd.BangError, match="`all` is out of range"):
            e.set_filters([0], np.array([1 << 32], np.int64))
        with pytest.raises(bang_amd.BangError, match="integers"):
            e.set_filters([0.5], [0])
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):        # bit 31 is a label like any other
            e.set_filters([1 << 31], [0xFFFFFFFF])
        s = e.stats()
        assert s["labelled"] == 0 and s["filtered_queries"] == 0 and s["label_launches"] == 0 and "excluded" in s
    finally:
        e.close()


def test_header_and_ctypes_mirrors_agree(tmp_path):
    """The layout program of tests/test_cabi.py on bang_label_filter and bang_stats_ext3; bang_search_params has the size it had, d_lut still its
    last member, and the earlier statistics structs keep size and offsets."""
    from bang_amd import binding as B
    assert B.StatsExt3._fields_[:-3] == B.StatsExt2._fields_
    assert B.StatsExt3._fields_[-3:] == [("labelled", C.c_uint64), ("filtered_queries", C.c_uint64), ("label_launches", C.c_uint64)]
    assert C.sizeof(B.StatsExt3) == C.sizeof(B.StatsExt2) + 24 and B.StatsExt3.labelled.offset == C.sizeof(B.StatsExt2)
    assert B.SearchParams._fields_[-1][0] == "d_lut" and C.sizeof(B.SearchParams) == SEARCH_PARAMS_SIZE
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*bang_stats_ext2 ext2;\s*uint64_t labelled;\s*uint64_t filtered_queries;\s*uint64_t label_launches;\s*\}\s*bang_stats_ext3;", hdr)
    assert re.search(r"typedef struct \{\s*const uint32_t\* d_labels;\s*const uint32_t\* d_filters;\s*const uint32_t\* d_excluded;\s*uint32_t\* d_matched;\s*\}\s*"
                     r"bang_label_filter;", hdr)
    assert re.search(r"const float\* d_lut;\s*\}\s*bang_search_params;", hdr)
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bang_c.h"', 'int main(void) {',
           '  printf("%zu %zu %zu %zu\\n", sizeof(bang_search_params), offsetof(bang_search_params, d_lut), sizeof(bang_stats_ext2), sizeof(bang_stats_ext3));',
           '  printf("%zu %zu %zu\\n", offsetof(bang_stats_ext3, labelled), offsetof(bang_stats_ext3, filtered_queries), offsetof(bang_stats_ext3, label_launches));',
           '  printf("%zu %zu %zu %zu %zu\\n", sizeof(bang_label_filter), offsetof(bang_label_filter, d_labels), offsetof(bang_label_filter, d_filters), '
           'offsetof(bang_label_filter, d_excluded), offsetof(bang_label_filter, d_matched));', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(c)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    L, S3 = B.LabelFilter, B.StatsExt3
    assert B.SearchParams.d_lut.offset == D_LUT_OFFSET
    assert got == [SEARCH_PARAMS_SIZE, D_LUT_OFFSET, C.sizeof(B.StatsExt2), C.sizeof(S3), S3.labelled.offset, S3.filtered_queries.offset,
                   S3.label_launches.offset, C.sizeof(L), L.d_labels.offset, L.d_filters.offset, L.d_excluded.offset, L.d_matched.offset]


def test_header_documents_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for decl in (r"bang_set_labels_e\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*labels\s*,\s*uint64_t\s+n\s*\)",
                 r"bang_clear_labels_e\s*\(\s*bang_engine_t\s*\*\s*e\s*\)",
                 r"bang_set_query_filters_e\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*any\s*,\s*const\s+uint32_t\s*\*\s*all\s*,\s*int\s+nq\s*\)",
                 r"bang_clear_query_filters_e\s*\(\s*bang_engine_t\s*\*\s*e\s*\)",
                 r"bang_k_search_exact_labels\s*\(\s*const\s+bang_search_params\s*\*\s*p\s*,\s*const\s+bang_label_filter\s*\*\s*f\s*,\s*void\s*\*\s*stream\s*\)",
                 r"bang_get_matched_counts\s*\(", r"bang_get_stats_ext3\s*\(", r"bang_search_exact_labels_geometry\s*\(", r"bang_search_exact_labels_pull_geometry\s*\("):
        assert re.search(r"^int\s+" + decl, src, flags=re.M), decl
    text = hdr[hdr.index("LABELS AND PER-QUERY FILTERS"):hdr.index("int bang_set_labels_e(")]
    for word in ("REPLACES", "n = 0 clears", "allocation is live", "bang_unload_e", "bit for bit", "capacity L", "UINT64_MAX", "\"labels\"", "\"filters\"",
                 "beam > 1", "vectors_fp16 = 1", "distance = 0", "BANG_LABEL_FILE", "BANG_QUERY_FILTER_FILE", "bang_k_worklist_pick is not launched"):
        assert word in text, word
    text = hdr[hdr.index("LABEL FILTERS on the exact-distance walk"):hdr.index("int bang_k_search_exact_labels(")]
    for word in ("MATCHES", "input order", "not the cap iteration", "strictly closer", "new before equal old", "first min(n, L)", "in twice", "d_matched",
                 "no member added or moved", "before any HIP call", "n_nodes == 0", "BANG_ERR_UNSUPPORTED"):
        assert word in text, word


def test_the_switches_are_in_the_option_table(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    assert "BANG_LABEL_FILE" in buf.value.decode() and "BANG_QUERY_FILTER_FILE" in buf.value.decode()


@pytest.mark.parametrize("obj,kernel", [("bang_search_exact_labels.o", "search_exact_labels_kernel"),
                                        ("bang_search_exact_labels_pull.o", "search_exact_labels_pull_kernel")])
def test_label_instances_run_without_scratch(libbang, tmp_path, obj, kernel):
    """One instance per vector type in each of the two new builds of the source: no scratch, no spill, and at most 128 VGPRs -- four waves per SIMD,
    the 16 waves per CU of the narrow instances -- read from the code object's kernel descriptors."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", obj)
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        m = re.match(r"_Z\d+" + kernel + r"ILi(\d)EEv9ExactArgs$", blk.split()[0])
        if m:
            found[int(m.group(1))] = tuple(int(re.search(r"\." + key + r":\s*(\d+)", blk).group(1))
                                           for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count"))
    assert sorted(found) == [0, 1, 2], found
    assert all(v[0] == 0 and v[1] == 0 and v[2] <= 128 for v in found.values()), found
