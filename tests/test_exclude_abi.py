"""C-ABI of the excluded ids (lazy deletes: bang_set_excluded_e / bang_clear_excluded_e, bang_k_cand_live / bang_k_worklist_pick of
csrc/bang_exclude.hip), without a GPU: the symbols are exported and documented, a broken contract is refused with BANG_ERR_ARG and a message
naming the member BEFORE any HIP call (on a machine without a device a launcher that reached the runtime would return BANG_ERR_HIP), the new
kernels use no scratch and no flat_ instruction, and the statistics structs before bang_stats_ext2 are what they were."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG = 0, -1
P = 0x1000                       # a non-null "device pointer": never dereferenced on the host


def _live(libbang, **over):
    a = dict(d_cand_ids=P, d_cand_cnt=P, cand_stride=87, q0=0, nq=4, d_bitmap=P, n_nodes=4000, d_live_ids=0x2000, d_live_cnt=P)
    a.update(over)
    f = libbang.bang_k_cand_live
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(a["d_cand_ids"], a["d_cand_cnt"], a["cand_stride"], a["q0"], a["nq"], a["d_bitmap"], a["n_nodes"], a["d_live_ids"], a["d_live_cnt"], None)
    return rc, libbang.bang_last_error().decode()


def _pick(libbang, **over):
    a = dict(d_wl_ids=P, d_wl_dists=P, L=37, q0=0, nq=4, Q_total=4, d_bitmap=P, n_nodes=4000, k=10, d_ids_out=0x2000, d_dists_out=0x2000)
    a.update(over)
    f = libbang.bang_k_worklist_pick
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                  C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(a["d_wl_ids"], a["d_wl_dists"], a["L"], a["q0"], a["nq"], a["Q_total"], a["d_bitmap"], a["n_nodes"], a["k"], a["d_ids_out"],
           a["d_dists_out"], None)
    return rc, libbang.bang_last_error().decode()


def test_symbols_are_exported(libbang):
    for name in ("bang_set_excluded_e", "bang_clear_excluded_e", "bang_k_cand_live", "bang_k_worklist_pick", "bang_get_stats_ext2"):
        assert hasattr(libbang, name), name


@pytest.mark.parametrize("over,member", [
    (dict(d_cand_ids=None), "d_cand_ids"),
    (dict(d_cand_cnt=None), "d_cand_cnt"),
    (dict(d_bitmap=None), "d_bitmap"),
    (dict(d_live_ids=None), "d_live_ids"),
    (dict(d_live_cnt=None), "d_live_cnt"),
    (dict(d_live_ids=P), "d_live_ids"),                     # the log itself: it stays the walk's
    (dict(cand_stride=0), "cand_stride"),
    (dict(q0=0xFFFFFFFF, nq=2), "q0"),
])
def test_cand_live_refuses_a_broken_contract(libbang, over, member):
    for extra in (dict(), dict(nq=0) if "nq" not in over else dict()):          # (checked before an empty batch is waved through)
        rc, err = _live(libbang, **dict(over, **extra))
        assert rc == ERR_ARG, (rc, err)
        assert member in err and "bang_k_cand_live" in err, err


@pytest.mark.parametrize("over,member", [
    (dict(d_wl_ids=None), "d_wl_ids"),
    (dict(d_wl_dists=None), "d_wl_dists"),
    (dict(d_bitmap=None), "d_bitmap"),
    (dict(d_ids_out=None), "d_ids_out"),
    (dict(d_dists_out=None), "d_dists_out"),
    (dict(d_ids_out=P), "d_ids_out"),                       # the outputs must not be the inputs
    (dict(k=0), "k = 0"),
    (dict(k=38), "k = 38"),
    (dict(L=0), "L = 0"),
    (dict(L=513, k=10), "L = 513"),
    (dict(Q_total=0), "Q_total"),
    (dict(Q_total=3), "Q_total"),
    (dict(q0=2, nq=3), "Q_total"),
])
def test_worklist_pick_refuses_a_broken_contract(libbang, over, member):
    for extra in (dict(), dict(nq=0) if "nq" not in over and over.get("Q_total") != 3 else dict()):
        rc, err = _pick(libbang, **dict(over, **extra))
        assert rc == ERR_ARG, (rc, err)
        assert member in err and "bang_k_worklist_pick" in err, err


def test_an_empty_batch_is_no_launch(libbang):
    assert _live(libbang, nq=0)[0] == OK
    assert _pick(libbang, nq=0)[0] == OK
    assert _pick(libbang, nq=0, k=37)[0] == OK              # k = L is allowed


def test_engine_calls_need_a_loaded_index(libbang):
    """Both calls are refused, with a message, on an engine without an index -- before any device call."""
    h = C.c_void_p()
    assert libbang.bang_create(0, C.byref(h)) == 0
    setx = libbang.bang_set_excluded_e
    setx.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    clr = libbang.bang_clear_excluded_e
    clr.argtypes = [C.c_void_p]
    ids = np.array([1, 2, 3], np.uint32)
    assert setx(h, ids.ctypes.data_as(C.c_void_p), 3) == ERR_ARG and "no index is loaded" in libbang.bang_last_error().decode()
    assert clr(h) == ERR_ARG and "no index is loaded" in libbang.bang_last_error().decode()
    assert setx(None, None, 0) == ERR_ARG and clr(None) == ERR_ARG
    libbang.bang_destroy.argtypes = [C.c_void_p]
    libbang.bang_destroy(h)


def test_python_binding_checks_the_ids_itself(libbang):
    import bang_amd
    assert callable(bang_amd.Engine.set_excluded) and callable(bang_amd.Engine.clear_excluded)
    e = bang_amd.Engine("uint8")
    try:
        with pytest.raises(bang_amd.BangError, match="out of range"):
            e.set_excluded([3, -1])
        with pytest.raises(bang_amd.BangError, match="out of range"):
            e.set_excluded(np.array([1 << 32], np.int64))
        with pytest.raises(bang_amd.BangError, match="integers"):
            e.set_excluded([0.5])
        with pytest.raises(bang_amd.BangError, match="no index is loaded"):
            e.set_excluded(np.array([5], np.int16))
    finally:
        e.close()


def test_statistics_are_appended_behind_the_structs_that_were(libbang, tmp_path):
    """bang_stats and bang_stats_ext keep size and offsets; `excluded` and `exclude_launches` are the last two fields of the statistics, in
    bang_stats_ext2.  Header and ctypes mirror agree (a C program prints the layout)."""
    from bang_amd import binding as B
    assert B.StatsExt2._fields_[:-2] == B.StatsExt._fields_
    assert B.StatsExt2._fields_[-2:] == [("excluded", C.c_uint64), ("exclude_launches", C.c_uint64)]
    assert C.sizeof(B.StatsExt2) == C.sizeof(B.StatsExt) + 16 and B.StatsExt2.excluded.offset == C.sizeof(B.StatsExt)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*bang_stats_ext ext;\s*uint64_t excluded;\s*uint64_t exclude_launches;\s*\}\s*bang_stats_ext2;", hdr)
    assert libbang.bang_get_stats_ext2(None, None) == ERR_ARG
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc:
        c = tmp_path / "layout.c"
        c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bang_c.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                     'sizeof(bang_stats_ext), sizeof(bang_stats_ext2), offsetof(bang_stats_ext2, excluded), '
                     'offsetof(bang_stats_ext2, exclude_launches)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(c)])
        got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
        assert got == [C.sizeof(B.StatsExt), C.sizeof(B.StatsExt2), B.StatsExt2.excluded.offset, B.StatsExt2.exclude_launches.offset]


def test_header_documents_the_entry_points(libbang):
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"^int\s+bang_set_excluded_e\s*\(\s*bang_engine_t\s*\*\s*e\s*,\s*const\s+uint32_t\s*\*\s*ids\s*,\s*uint64_t\s+n\s*\)", src, flags=re.M)
    assert re.search(r"^int\s+bang_clear_excluded_e\s*\(\s*bang_engine_t\s*\*\s*e\s*\)", src, flags=re.M)
    for name in ("bang_k_cand_live", "bang_k_worklist_pick", "bang_get_stats_ext2"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
    text = hdr[hdr.index("EXCLUDED IDS (lazy deletes"):hdr.index("int bang_set_excluded_e(")]
    for word in ("REPLACES", "n = 0 clears", "out of range", "allocation is live", "bang_unload_e", "rerank_fused", "UINT64_MAX", "BANG_EXCLUDE_FILE",
                 "\"excluded\"", "bit for bit"):
        assert word in text, word
    text = hdr[hdr.index("EXCLUDED IDS, device side"):hdr.index("int bang_k_worklist_pick(")]
    for word in ("d_bitmap", "slack", "n_nodes", "before any HIP call", "BANG_ERR_ARG", "log order", "d_live_cnt", "rr_k = L", "worklist order",
                 "ends the scan", "must not be the inputs"):
        assert word in text, word


def test_the_switch_is_in_the_option_table(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    assert "BANG_EXCLUDE_FILE" in buf.value.decode()


def test_kernels_use_no_scratch_no_lds_and_no_flat_instruction(libbang, tmp_path):
    """The gfx950 code object of bang_exclude.o: both kernels with .private_segment_fixed_size == 0 and no LDS, and not one flat_ / scratch_
    instruction in the object."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_exclude.o")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        m = re.match(r"_Z\d+(cand_live_kernel|worklist_pick_kernel)\d+\w+Args$", blk.split()[0])
        if m:
            found[m.group(1)] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)),
                                 int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)))
    assert sorted(found) == ["cand_live_kernel", "worklist_pick_kernel"], found
    assert all(v == (0, 0) for v in found.values()), found
    assert all(int(x) == 0 for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", notes)), notes
    asm = subprocess.run([tools[3], "-d", co], check=True, capture_output=True, text=True).stdout
    assert "global_load_dword" in asm and "v_mbcnt_hi_u32_b32" in asm
    assert not re.search(r"\b(flat|scratch)_\w+", asm)
