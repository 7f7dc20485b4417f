"""Option vectors_fp16 without a GPU: the option table, the C-ABI members it adds (bang_stats.vectors_fp16 / vector_table_bytes,
bang_search_params.rr_vec_f16, bang_k_f32_to_f16, bang_k_rerank_f16) and the argument checks of bang_k_search_exact with rr_vec_f16 = 1 --
refused with the right code and a message naming the member BEFORE any HIP call (a launcher that reached the runtime on a machine without a
device would return BANG_ERR_HIP, not the code asserted here)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
U8, I8, F32 = 0, 1, 2


def _option_table(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    return buf.value.decode()


def test_option_is_in_the_table_and_takes_0_or_1(libbang):
    text = _option_table(libbang)
    row = re.search(r"^  vectors_fp16\s+BANG_VECTORS_FP16\s+\[0, 1\]\s+bang_load\s", text, flags=re.M)
    assert row, text[:400]
    h = C.c_void_p()
    assert libbang.bang_create(F32, C.byref(h)) == 0
    libbang.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    libbang.bang_destroy.argtypes = [C.c_void_p]
    try:
        for v in (0, 1):
            assert libbang.bang_set_option(h, b"vectors_fp16", v) == OK
        for v in (2, -1):
            assert libbang.bang_set_option(h, b"vectors_fp16", v) == ERR_ARG
            assert "vectors_fp16" in libbang.bang_last_error().decode()
    finally:
        libbang.bang_destroy(h)


def test_engine_takes_the_option_through_its_keywords(libbang):
    import bang_amd
    with bang_amd.Engine("float", vectors_fp16=1) as e:
        e.set_option("vectors_fp16", 0)
        with pytest.raises(bang_amd.BangError):
            e.set_option("vectors_fp16", 2)


def test_new_members_agree_between_header_and_binding(tmp_path):
    """The method of tests/test_cabi.py (a C program prints sizeof and offsetof) on the members this option adds.  bang_stats: appended last.
    bang_search_params: rr_vec_f16 takes the four bytes of padding that lay between rr_Q_total and d_lut, so NO member moved, d_lut is still the
    last one and sizeof is what it was."""
    from bang_amd import binding as B
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    pairs = {"bang_stats": B.Stats, "bang_search_params": B.SearchParams}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bang_c.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = line.split()
        got[(s, f)] = int(v)
    for cname, cls in pairs.items():
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, f"{cname}.{f}"
    st = [f for f, _ in B.Stats._fields_]
    assert st[-3:] == ["rerank_fused", "vectors_fp16", "vector_table_bytes"] and got[("bang_stats", "size")] == got[("bang_stats", "vector_table_bytes")] + 8
    assert dict(B.Stats._fields_)["vectors_fp16"] is C.c_uint64 and dict(B.SearchParams._fields_)["rr_vec_f16"] is C.c_uint32
    sp = "bang_search_params"
    assert got[(sp, "rr_vec_f16")] == got[(sp, "rr_Q_total")] + 4 and got[(sp, "d_lut")] == got[(sp, "rr_vec_f16")] + 4
    assert got[(sp, "size")] == got[(sp, "d_lut")] + 8


def test_kernel_level_entries_are_declared_and_exported(libbang):
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    for name in ("bang_k_f32_to_f16", "bang_k_rerank_f16", "bang_search_exact_pull_f16_geometry"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert hasattr(libbang, name), name
    decl = re.search(r"int bang_k_f32_to_f16\((.*?)\);", hdr, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["d_src", "d_dst", "rows", "D", "src_stride", "dst_stride", "d_bad_count", "stream"]


def test_conversion_entry_checks_its_arguments_before_any_launch(libbang):
    fn = libbang.bang_k_f32_to_f16
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    assert fn(0x1000, 0x2000, 0, 8, 32, 16, None, None) == OK                 # no rows: no launch
    for args in ((None, 0x2000, 4, 8, 32, 16), (0x1000, 0x2002, 4, 8, 32, 16), (0x1000, 0x2000, 4, 8, 28, 16), (0x1000, 0x2000, 4, 8, 32, 12),
                 (0x1000, 0x2000, 4, 7, 28, 14), (0x1000, 0x2000, 4, 0, 32, 16)):
        assert fn(*args, None, None) == ERR_ARG, args
        assert "bang_k_f32_to_f16" in libbang.bang_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- bang_k_search_exact, rr_vec_f16
def _params(B, **over):
    """A pulled-rows launch on an fp16 table that passes every check (the pointers are never dereferenced on the host)."""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.L, sp.medoid, sp.cap_iter = 4, 32, 37, 0, 37 + 49
    sp.row_layout, sp.entry_len, sp.vec_bytes = 1, 256, 4 * 96
    sp.rr_dtype, sp.rr_D, sp.rr_k, sp.rr_q0, sp.rr_Q_total = F32, 96, 10, 0, 4
    sp.rr_vec_stride, sp.rr_vec_f16 = 2 * 96, 1
    for f in ("d_seed", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query", "rr_queries", "rr_vec_base", "rr_ids_out", "rr_dists_out"):
        setattr(sp, f, 0x1000)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


def _call(libbang, sp):
    f = libbang.bang_k_search_exact
    f.argtypes = [C.c_void_p, C.c_void_p]
    rc = f(C.byref(sp), None)
    return rc, libbang.bang_last_error().decode()


@pytest.mark.parametrize("over", [
    dict(rr_dtype=U8, rr_D=96, vec_bytes=96),
    dict(rr_dtype=I8, rr_D=128, vec_bytes=128),
    dict(rr_D=100, vec_bytes=400, rr_vec_stride=200),                 # D % 8 != 0
    dict(rr_D=260, vec_bytes=1040, rr_vec_stride=520),                # D > 256
    dict(rr_D=0, vec_bytes=0),
    dict(row_layout=0, entry_len=4 * 96 + 4 + 4 * 32),                # graph entries in HBM hold float vectors
    dict(rr_vec_f16=2),
    dict(rr_vec_stride=190),                                          # not divisible by 4
    dict(rr_vec_stride=96),                                           # shorter than a row of halves
])
def test_fp16_rows_are_refused_where_no_instance_reads_them(libbang, over):
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, **over))
    assert rc == ERR_ARG, (rc, err)
    assert "rr_vec_f16" in err, err


def test_the_other_members_are_checked_as_before(libbang):
    """rr_vec_f16 = 1 changes what rr_vec_stride must hold and nothing else: the messages of the float form."""
    from bang_amd import binding as B
    for over, message in ((dict(rr_vec_base=None), "rr_vec_base"), (dict(vec_bytes=2 * 96), "vec_bytes"), (dict(n_rows_hbm=5), "d_rows_hbm"),
                          (dict(d_graph=0x1002), "d_graph"), (dict(n_slices=2), "d_row_slices")):
        rc, err = _call(libbang, _params(B, **over))
        assert rc == ERR_ARG and message in err, (over, rc, err)
    rc, _ = _call(libbang, _params(B, Q=0))
    assert rc == OK
    # rr_vec_f16 = 0: a float table of 2 * D bytes per row is no layout
    rc, err = _call(libbang, _params(B, rr_vec_f16=0))
    assert rc == ERR_ARG and "rr_vec_stride" in err, (rc, err)


def test_the_fp16_instance_is_one_kernel_without_scratch(libbang, tmp_path):
    """The fifth build of csrc/bang_search_exact.hip holds ONE kernel (float queries on fp16 rows), no scratch -- read from the code object."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_search_exact_pull_f16.o")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        m = re.match(r"_Z\d+search_exact\w*kernelILi(\d)EEv9ExactArgs$", blk.split()[0])
        if m:
            found[blk.split()[0]] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
    assert list(found) == ["_Z28search_exact_pull_f16_kernelILi2EEv9ExactArgs"], found
    assert all(v == 0 for v in found.values()), found


def test_documents_name_the_option(libbang):
    text = _option_table(libbang)
    entry = text[text.index("  vectors_fp16"):]
    entry = entry[:entry.index("\n  pull ")]
    for word in ("fp16", "distance = 1", "65520", "graph = device", "vectors = 0"):
        assert word in entry, word
    for doc, words in (("README.md", ("vectors_fp16",)), ("DESIGN.md", ("4.9", "vectors_fp16", "bf16")), ("INTEGRATION.md", ("BANG_VECTORS_FP16",))):
        body = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in body, (doc, w)
