"""C-ABI of range search (bang_k_search_exact_range, bang_k_range_sort, bang_set_query_radii_e, bang_get_range_counts / _results, bang_stats_ext4),
without a GPU: the symbols are exported and documented, a broken contract is refused with its code and a message naming the member BEFORE any HIP
call (on a machine without a device a launcher that reached the runtime would return BANG_ERR_HIP), header and ctypes mirrors agree on the new
structs while the earlier ones keep their size, the option is in the one table, and the new code objects hold their instances without scratch in at
most 128 VGPRs."""
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
SEARCH_PARAMS_SIZE, D_LUT_OFFSET = 376, 368     # bang_search_params as it was (tests/test_labels_abi.py)
MAX_HITS = 4096


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


def _range(B, **over):
    r = B.RangeOut()
    r.d_radius, r.d_excluded, r.d_hit_ids, r.d_hit_dists, r.d_offered, r.cap = P, None, P, P, P, 512
    for k, v in over.items():
        setattr(r, k, v)
    return r


def _call(libbang, sp, ro):
    f = libbang.bang_k_search_exact_range
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(C.byref(sp) if sp is not None else None, C.byref(ro) if ro is not None else None, None)
    return rc, libbang.bang_last_error().decode()


def _sort(libbang, ids=P, dists=P, offered=P, cap=512, q0=0, nq=4, Q_total=4, count=P):
    f = libbang.bang_k_range_sort
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(ids, dists, offered, cap, q0, nq, Q_total, count, None)
    return rc, libbang.bang_last_error().decode()


def test_symbols_are_exported(libbang):
    for name in ("bang_k_search_exact_range", "bang_search_exact_range_geometry", "bang_search_exact_range_pull_geometry", "bang_k_range_sort",
                 "bang_set_query_radii_e", "bang_clear_query_radii_e", "bang_get_range_counts", "bang_get_range_results", "bang_get_stats_ext4"):
        assert hasattr(libbang, name), name


@pytest.mark.parametrize("layout", (0, 1))
def test_range_arguments_are_refused_with_the_member_named(libbang, layout):
    from bang_amd import binding as B
    assert _call(libbang, None, _range(B))[0] == ERR_ARG
    for empty in (dict(), dict(Q=0)):                                  # (checked before an empty batch is waved through)
        rc, err = _call(libbang, _params(B, layout, **empty), None)
        assert rc == ERR_ARG and "bang_range_out" in err, (rc, err)
        for member in ("d_radius", "d_hit_ids", "d_hit_dists", "d_offered"):
            rc, err = _call(libbang, _params(B, layout, **empty), _range(B, **{member: None}))
            assert rc == ERR_ARG and member in err, (rc, err)
        for cap in (0, MAX_HITS + 1, 0xFFFFFFFF):
            rc, err = _call(libbang, _params(B, layout, **empty), _range(B, cap=cap))
            assert rc == ERR_ARG and "cap" in err and str(MAX_HITS) in err, (rc, err)
        rc, err = _call(libbang, _params(B, layout, n_nodes=0, **empty), _range(B, d_excluded=P))
        assert rc == ERR_ARG and "n_nodes" in err and "d_excluded" in err, (rc, err)
    assert _call(libbang, _params(B, layout, Q=0), _range(B))[0] == OK  # an empty batch is no launch at all
    assert _call(libbang, _params(B, layout, Q=0, n_nodes=0), _range(B, cap=MAX_HITS))[0] == OK     # (n_nodes = 0 without a bitmap is fine)


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
def test_every_check_of_the_plain_entry_is_made(libbang, layout, over, code, message):
    """The code and message bang_k_search_exact gives for the same arguments."""
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, layout, **over), _range(B))
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
    rc, err = _call(libbang, _params(B, layout, **over), _range(B))
    assert rc == ERR_UNSUPPORTED and message in err and "range" in err, (rc, err)


def test_range_sort_arguments_are_refused_with_the_argument_named(libbang):
    for name in ("ids", "dists", "offered", "count"):
        rc, err = _sort(libbang, **{name: None})
        assert rc == ERR_ARG and ("d_hit_" + name if name in ("ids", "dists") else "d_" + name) in err, (rc, err)
        rc, err = _sort(libbang, nq=0, **{name: None})                 # (checked before an empty batch is waved through)
        assert rc == ERR_ARG, (rc, err)
    for cap in (0, MAX_HITS + 1):
        rc, err = _sort(libbang, cap=cap)
        assert rc == ERR_ARG and "cap" in err, (rc, err)
    rc, err = _sort(libbang, q0=2, nq=3, Q_total=4)
    assert rc == ERR_ARG and "Q_total" in err, (rc, err)
    rc, err = _sort(libbang, q0=0xFFFFFFFF, nq=2, Q_total=0xFFFFFFFF)   # (q0 + nq does not wrap)
    assert rc == ERR_ARG and "Q_total" in err, (rc, err)
    assert _sort(libbang, nq=0)[0] == OK                                # no launch
    assert _sort(libbang, q0=4, nq=0, Q_total=4, cap=MAX_HITS)[0] == OK


def test_engine_calls_are_refused_without_an_allocation(libbang):
    """Every engine entry is refused, with a message, before any device call."""
    h = C.c_void_p()
    assert libbang.bang_create(0, C.byref(h)) == 0
    setr = libbang.bang_set_query_radii_e
    setr.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    clrr = libbang.bang_clear_query_radii_e
    clrr.argtypes = [C.c_void_p]
    getc = libbang.bang_get_range_counts
    getc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    getr = libbang.bang_get_range_results
    getr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    r = np.ones(3, np.float32)
    w = np.zeros(4, np.uint64)
    rp, wp = r.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    assert setr(h, rp, 3) == ERR_ARG and "bang_alloc" in libbang.bang_last_error().decode()
    assert clrr(h) == OK                                               # nothing to drop
    assert getc(h, wp, wp, 3) == ERR_ARG and "radii" in libbang.bang_last_error().decode()
    assert getr(h, wp, wp, wp, 3) == ERR_ARG and "radii" in libbang.bang_last_error().decode()
    assert setr(None, None, 0) == ERR_ARG and clrr(None) == ERR_ARG and getc(None, None, None, 0) == ERR_ARG
    assert getr(None, None, None, None, 0) == ERR_ARG and getr(h, None, wp, wp, 3) == ERR_ARG and libbang.bang_get_stats_ext4(None, None) == ERR_ARG
    libbang.bang_destroy.argtypes = [C.c_void_p]
    libbang.bang_destroy(h)


def test_python_binding(libbang):
    import bang_amd
    for name in ("set_radii", "clear_radii", "range_counts", "range_results"):
        assert callable(getattr(bang_amd.Engine, name)), name
    e = bang_amd.Engine("uint8", range_hits=512)                         # through the one option path
    try:
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):
            e.set_radii([1.0, 2.0])
        with pytest.raises(bang_amd.BangError, match="bang_alloc"):
            e.set_radii(3.0, Q=4)                                        # a scalar is broadcast
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.range_counts(4)
        with pytest.raises(bang_amd.BangError, match="radii"):
            e.range_results(4)
        e.clear_radii()
        s = e.stats()
        assert s["range_hits"] == 512 and s["range_queries"] == 0 and s["range_launches"] == 0 and s["range_truncated"] == 0 and "labelled" in s
        with pytest.raises(bang_amd.BangError, match="range_hits"):
            e.set_option("range_hits", 4097)
        with pytest.raises(bang_amd.BangError, match="range_hits"):
            e.set_option("range_hits", -1)
        e.set_option("range_hits", 0)
        assert e.stats()["range_hits"] == 0
    finally:
        e.close()


def test_the_environment_presets_the_option(libbang, monkeypatch):
    import bang_amd
    monkeypatch.setenv("BANG_RANGE_HITS", "100000")                      # clamped to the range, as every environment preset
    with bang_amd.Engine("uint8") as e:
        assert e.stats()["range_hits"] == MAX_HITS
    monkeypatch.setenv("BANG_RANGE_HITS", "64")
    with bang_amd.Engine("uint8") as e:
        assert e.stats()["range_hits"] == 64


def test_header_and_ctypes_mirrors_agree(tmp_path):
    """The layout program of tests/test_cabi.py on bang_range_out and bang_stats_ext4; bang_search_params has the size it had, d_lut still its last
    member, and the earlier statistics structs keep size and offsets."""
    from bang_amd import binding as B
    assert B.StatsExt4._fields_[:-4] == B.StatsExt3._fields_
    assert [f for f, _ in B.StatsExt4._fields_[-4:]] == ["range_hits", "range_queries", "range_launches", "range_truncated"]
    assert C.sizeof(B.StatsExt4) == C.sizeof(B.StatsExt3) + 32 and B.StatsExt4.range_hits.offset == C.sizeof(B.StatsExt3)
    assert B.SearchParams._fields_[-1][0] == "d_lut" and C.sizeof(B.SearchParams) == SEARCH_PARAMS_SIZE
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*bang_stats_ext3 ext3;\s*uint64_t range_hits;\s*uint64_t range_queries;\s*uint64_t range_launches;\s*"
                     r"uint64_t range_truncated;\s*\}\s*bang_stats_ext4;", hdr)
    assert re.search(r"typedef struct \{\s*const float\*\s+d_radius;\s*const uint32_t\*\s+d_excluded;\s*uint32_t\*\s+d_hit_ids;\s*float\*\s+d_hit_dists;\s*"
                     r"uint32_t\*\s+d_offered;\s*uint32_t\s+cap;\s*\}\s*bang_range_out;", hdr)
    assert re.search(r"#define BANG_RANGE_MAX_HITS 4096u", hdr)
    assert re.search(r"const float\* d_lut;\s*\}\s*bang_search_params;", hdr)
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bang_c.h"', 'int main(void) {',
           '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bang_search_params), offsetof(bang_search_params, d_lut), sizeof(bang_stats), sizeof(bang_stats_ext), '
           'sizeof(bang_stats_ext2), sizeof(bang_stats_ext3), sizeof(bang_stats_ext4));',
           '  printf("%zu %zu %zu %zu\\n", offsetof(bang_stats_ext4, range_hits), offsetof(bang_stats_ext4, range_queries), offsetof(bang_stats_ext4, range_launches), '
           'offsetof(bang_stats_ext4, range_truncated));',
           '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bang_range_out), offsetof(bang_range_out, d_radius), offsetof(bang_range_out, d_excluded), '
           'offsetof(bang_range_out, d_hit_ids), offsetof(bang_range_out, d_hit_dists), offsetof(bang_range_out, d_offered), offsetof(bang_range_out, cap));',
           '  printf("%zu %u\\n", sizeof(bang_label_filter), BANG_RANGE_MAX_HITS);', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(c)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    R, S4 = B.RangeOut, B.StatsExt4
    assert got == [SEARCH_PARAMS_SIZE, D_LUT_OFFSET, C.sizeof(B.Stats), C.sizeof(B.StatsExt), C.sizeof(B.StatsExt2), C.sizeof(B.StatsExt3), C.sizeof(S4),
                   S4.range_hits.offset, S4.range_queries.offset, S4.range_launches.offset, S4.range_truncated.offset,
                   C.sizeof(R), R.d_radius.offset, R.d_excluded.offset, R.d_hit_ids.offset, R.d_hit_dists.offset, R.d_offered.offset, R.cap.offset,
                   C.sizeof(B.LabelFilter), MAX_HITS]
    assert C.sizeof(R) == 48 and R.cap.offset == 40


def test_header_documents_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for decl in (r"bang_set_query_radii_e\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*const\s+float\s*\*\s*radii\s*,\s*int\s+nq\s*\)",
                 r"bang_clear_query_radii_e\s*\(\s*bang_engine_t\s*\*\s*e\s*\)",
                 r"bang_get_range_counts\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*uint32_t\s*\*\s*counts\s*,\s*uint32_t\s*\*\s*offered\s*,\s*uint32_t\s+num_queries\s*\)",
                 r"bang_get_range_results\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*uint64_t\s*\*\s*lims\s*,\s*uint64_t\s*\*\s*ids\s*,\s*float\s*\*\s*dists\s*,\s*uint64_t\s+capacity\s*\)",
                 r"bang_k_search_exact_range\s*\(\s*const\s+bang_search_params\s*\*\s*p\s*,\s*const\s+bang_range_out\s*\*\s*r\s*,\s*void\s*\*\s*stream\s*\)",
                 r"bang_k_range_sort\s*\(\s*uint32_t\s*\*\s*d_hit_ids\s*,\s*float\s*\*\s*d_hit_dists\s*,\s*const\s+uint32_t\s*\*\s*d_offered\s*,\s*uint32_t\s+cap\s*,\s*"
                 r"uint32_t\s+q0\s*,\s*uint32_t\s+nq\s*,\s*uint32_t\s+Q_total\s*,\s*uint32_t\s*\*\s*d_count\s*,\s*void\s*\*\s*stream\s*\)",
                 r"bang_get_stats_ext4\s*\(", r"bang_search_exact_range_geometry\s*\(", r"bang_search_exact_range_pull_geometry\s*\("):
        assert re.search(r"^int\s+" + decl, src, flags=re.M), decl
    text = hdr[hdr.index("RANGE SEARCH (DESIGN.md"):hdr.index("int bang_set_query_radii_e(")]
    for word in ("range_hits", "bit for bit", "cap iteration", "NaN or negative", "+inf", "evaluation order", "nq = 0 clears", "\"radii\"", "\"range\"",
                 "label filters together are refused", "distance = 0", "beam > 1", "vectors_fp16 = 1", "lims[0] = 0", "nothing is written", "truncated"):
        assert word in text, word
    text = hdr[hdr.index("RANGE SEARCH on the exact-distance walk"):hdr.index("int bang_k_search_exact_range(")]
    for word in ("EVERY iteration", "input order", "element 64", "d_offered", "no member added or moved", "before any HIP call", "n_nodes == 0",
                 "BANG_ERR_UNSUPPORTED", "BANG_RANGE_MAX_HITS"):
        assert word in text, word


def test_the_option_is_in_the_one_table(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    rows = [l for l in buf.value.decode().splitlines() if l.startswith("  range_hits ")]
    assert len(rows) == 1
    assert "BANG_RANGE_HITS" in rows[0] and "[0, 4096]" in rows[0] and "bang_alloc" in rows[0] and "0 = off (default)" in rows[0]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert rows[0] in integration                                       # (INTEGRATION.md carries the table verbatim)


def _kernel_figures(tmp_path, obj):
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
    out = {}
    for blk in notes.split(".name:")[1:]:
        out[blk.split()[0]] = tuple(int(re.search(r"\." + key + r":\s*(\d+)", blk).group(1))
                                    for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count"))
    return out


@pytest.mark.parametrize("obj,kernel", [("bang_search_exact_range.o", "search_exact_range_kernel"),
                                        ("bang_search_exact_range_pull.o", "search_exact_range_pull_kernel")])
def test_range_instances_run_without_scratch(libbang, tmp_path, obj, kernel):
    """One instance per vector type in each of the two new builds of the source: no scratch, no spill, and at most 128 VGPRs -- four waves per SIMD,
    the 16 waves per CU of the narrow instances -- read from the code object's kernel descriptors."""
    found = {}
    for name, v in _kernel_figures(tmp_path, obj).items():
        m = re.match(r"_Z\d+" + kernel + r"ILi(\d)EEv9ExactArgs$", name)
        if m:
            found[int(m.group(1))] = v
    assert sorted(found) == [0, 1, 2], found
    assert all(v[0] == 0 and v[1] == 0 and v[2] <= 128 for v in found.values()), found


def test_range_sort_kernel_runs_without_scratch(libbang, tmp_path):
    found = {n: v for n, v in _kernel_figures(tmp_path, "bang_range.o").items() if "range_sort_kernel" in n}
    assert len(found) == 1 and all(v[0] == 0 and v[1] == 0 and v[2] <= 64 for v in found.values()), found
