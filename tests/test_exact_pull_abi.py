"""C-ABI of the exact-distance search kernel's pulled-rows form (bang_search_params.row_layout = 1: 256-byte adjacency rows in d_graph, the
vectors at rr_vec_base + id * rr_vec_stride), without a GPU: bang_k_search_exact refuses what breaks the contract of include/bang_c.h with
the right code and a message naming the member BEFORE any HIP call (on a machine without a device a launcher that reached the runtime would
return BANG_ERR_HIP, not the code asserted here), the code object holds the pulled instances without scratch, and the option table
describes the mode."""
import ctypes as C
import os
import re
import subprocess

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


def _call(libbang, sp):
    f = libbang.bang_k_search_exact
    f.argtypes = [C.c_void_p, C.c_void_p]
    rc = f(C.byref(sp), None)
    return rc, libbang.bang_last_error().decode()


@pytest.mark.parametrize("over,message", [
    (dict(rr_vec_base=None), "rr_vec_base"),
    (dict(rr_vec_base=0x1002), "rr_vec_base"),
    (dict(rr_vec_stride=0), "rr_vec_stride"),
    (dict(rr_vec_stride=126), "rr_vec_stride"),                       # not divisible by 4
    (dict(rr_vec_stride=64), "rr_vec_stride"),                        # shorter than the vector
    (dict(rr_dtype=F32, rr_D=128, vec_bytes=512, rr_vec_stride=256), "rr_vec_stride"),
    (dict(rr_D=40, vec_bytes=40, rr_vec_stride=40), "rr_vec_stride"),  # 8-bit vectors with D % 16 != 0: no layout of bang_search_exact_supported
    (dict(vec_bytes=0), "vec_bytes"),
    (dict(rr_dtype=F32, rr_D=32, vec_bytes=32), "vec_bytes"),
    (dict(n_slices=2), "d_row_slices"),
    (dict(n_slices=2, d_row_slices=0x1000), "slice_rows"),
    (dict(n_rows_hbm=5), "d_rows_hbm"),
    (dict(R=65), "R"),
    (dict(d_graph=None), "d_graph"),
    (dict(d_graph=0x1002), "d_graph"),
])
def test_pulled_form_refuses_a_broken_contract(libbang, over, message):
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, **over))
    assert rc == ERR_ARG, (rc, err)
    assert message in err, err


def test_other_row_layouts_stay_unsupported(libbang):
    from bang_amd import binding as B
    for layout in (2, 7):
        rc, err = _call(libbang, _params(B, row_layout=layout))
        assert rc == ERR_UNSUPPORTED and "row_layout" in err, (rc, err)


def test_graph_entry_form_is_checked_as_before(libbang):
    """row_layout = 0: the messages of the parent commit."""
    from bang_amd import binding as B
    rc, err = _call(libbang, _params(B, row_layout=0, d_graph=None, entry_len=128 + 4 * 33))
    assert rc == ERR_UNSUPPORTED and "needs the graph entries in HBM (d_graph, row_layout = 0)" in err
    rc, err = _call(libbang, _params(B, row_layout=0, entry_len=130, rr_vec_base=None, rr_vec_stride=0))
    assert rc == ERR_UNSUPPORTED and "unsupported vector layout" in err
    rc, err = _call(libbang, _params(B, row_layout=0, entry_len=128 + 4 * 33, R=65))
    assert rc == ERR_ARG and "bad R/L" in err


def test_null_and_empty(libbang):
    from bang_amd import binding as B
    f = libbang.bang_k_search_exact
    f.argtypes = [C.c_void_p, C.c_void_p]
    assert f(None, None) == ERR_ARG
    rc, _ = _call(libbang, _params(B, Q=0, rr_vec_base=None))           # an empty batch is no launch at all
    assert rc == OK


def test_header_documents_the_pulled_form():
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    text = hdr[hdr.index("EXACT-DISTANCE search kernel"):hdr.index("int bang_k_search_exact(")]
    for word in ("row_layout = 1", "rr_vec_base", "rr_vec_stride", "d_rows_hbm", "d_row_slices", "BANG_ERR_ARG"):
        assert word in text, word


def test_option_table_mentions_the_pulled_form(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    text = buf.value.decode()
    entry = text[text.index("  distance"):]
    entry = entry[:entry.index("\n  semantics")]
    assert "pull = 1" in entry and "graph = host" in entry, entry


@pytest.mark.parametrize("obj,kernel", [("bang_search_exact_pull.o", "search_exact_pull_kernel"), ("bang_search_exact_wide_pull.o", "search_exact_wide_pull_kernel")])
def test_pulled_instances_run_without_scratch(libbang, tmp_path, obj, kernel):
    """One pulled instance per vector type in each of the two further builds of the source, no scratch -- read from the code object's kernel descriptors."""
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
            found[int(m.group(1))] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
    assert sorted(found) == [0, 1, 2], found
    assert all(v == 0 for v in found.values()), found
