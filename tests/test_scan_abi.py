"""The exact scan's ABI without a GPU: the exports exist, every refusal that needs no device comes with its code and message before any HIP call
and leaves the output buffers alone, the two test hooks live in the environment table, the host side (csrc/bang_scan_host.cpp, no HIP call) is
built with a stand-alone main under -fsanitize=address,undefined and run as a program (no Python runs under a sanitizer), and the cross-compiled
kernels use no private segment."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5


def _err(lib):
    lib.bang_last_error.restype = C.c_char_p
    return lib.bang_last_error().decode()


def test_exports(libbang):
    for sym in ("bang_scan_e", "bang_get_scan_times", "bang_k_scan", "bang_scan_geometry", "bang_scan_max_stripes", "bang_scan_scratch_bytes",
                "bang_scan_check", "bang_k_bitmap_or"):
        getattr(libbang, sym)
    from bang_amd import binding as B
    assert callable(B.Engine.scan) and callable(B.Engine.scan_times)
    hdr = open(os.path.join(ROOT, "include", "bang_c.h")).read()
    assert re.search(r"#define BANG_SCAN_MAX_K 128u", hdr)


def test_the_hooks_are_in_the_environment_table(libbang):
    libbang.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = libbang.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    libbang.bang_describe_options(buf, need)
    text = buf.value.decode()
    for hook in ("BANG_SCAN_STRIPES", "BANG_SCAN_QUERY_CHUNK"):
        rows = [l for l in text.splitlines() if hook in l]
        assert len(rows) == 1 and "test hook" in rows[0] and "clamped" in rows[0], rows


def _scan(lib, h, q, nq, k, any_, all_, ids, dists, matched):
    lib.bang_scan_e.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    return lib.bang_scan_e(h, p(q), nq, k, p(any_), p(all_), p(ids), p(dists), p(matched))


def test_engine_refusals_that_need_no_device(libbang):
    lib = libbang
    q = np.zeros((4, 128), np.uint8)
    ids = np.full((4, 10), 7, np.uint64)
    dists = np.full((10, 4), 7.0, np.float32)
    matched = np.full(4, 7, np.uint32)
    assert _scan(lib, None, q, 4, 10, None, None, ids, dists, matched) == ERR_ARG and "bang_scan" in _err(lib) and "null" in _err(lib)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    # nothing is loaded: said first, whatever else is wrong with the call
    for nq, k, a in ((4, 10, None), (0, 10, None), (4, 129, None), (4, 10, np.zeros(4, np.uint32))):
        assert _scan(lib, h, q, nq, k, a, None, ids, dists, matched) == ERR_ARG and "bang_scan" in _err(lib) and "no index is loaded" in _err(lib)
    assert (ids == 7).all() and (dists == 7.0).all() and (matched == 7).all(), "a refused call wrote an output buffer"
    lib.bang_get_scan_times.argtypes = [C.c_void_p, C.c_void_p]
    ms = (C.c_double * 3)(1, 1, 1)
    assert lib.bang_get_scan_times(h, None) == ERR_ARG and lib.bang_get_scan_times(None, ms) == ERR_ARG
    assert lib.bang_get_scan_times(h, ms) == OK and list(ms) == [0, 0, 0]
    lib.bang_destroy.argtypes = [C.c_void_p]
    lib.bang_destroy(h)


_GOOD = dict(d_vec_base=0x10000, vec_stride=128 + 4 + 4 * 64, dtype=0, D=128, n_nodes=4000, d_queries=0x20000, nq=64, k=10, stripes=2,
             d_scratch=0x30000, scratch_bytes=8 * 64 * 2 * 10 + 8 * 64, d_ids_out=0x40000, d_dists_out=0x50000, d_matched=0x60000)
_REFUSALS = [
    (dict(d_vec_base=None), ERR_ARG, "d_vec_base"), (dict(d_vec_base=0x10002), ERR_ARG, "d_vec_base"), (dict(d_queries=None), ERR_ARG, "d_queries"),
    (dict(n_nodes=0), ERR_ARG, "n_nodes"), (dict(nq=0), ERR_ARG, "nq = 0"), (dict(nq=(1 << 20) + 1), ERR_ARG, "nq"), (dict(k=0), ERR_ARG, "k = 0"),
    (dict(k=129), ERR_ARG, "k = 129"),
    (dict(D=48), ERR_UNSUPPORTED, "layout"),                               # 8-bit D / 16 = 3: a wide layout
    (dict(D=320, dtype=2, vec_stride=4 * 320 + 260), ERR_UNSUPPORTED, "layout"),
    (dict(vec_stride=64), ERR_UNSUPPORTED, "layout"),                      # the stride does not hold the vector
    (dict(vec_stride=390), ERR_UNSUPPORTED, "layout"), (dict(dtype=3), ERR_UNSUPPORTED, "layout"),
    (dict(d_labels=0x70000), ERR_ARG, "d_labels"), (dict(d_filters=0x70000), ERR_ARG, "d_filters"),
    (dict(stripes=33), ERR_ARG, "stripes"),                                # ceil(4000 / 128) = 32 rounds
    (dict(k=128, stripes=33, scratch_bytes=1 << 30), ERR_ARG, "stripes"),  # and 33 x 128 keys > 4096
    (dict(d_scratch=None), ERR_ARG, "d_scratch"), (dict(d_scratch=0x30004), ERR_ARG, "d_scratch"),
    (dict(scratch_bytes=8 * 64 * 2 * 10 + 8 * 64 - 1), ERR_ARG, "scratch_bytes"),
    (dict(d_ids_out=None), ERR_ARG, "d_ids_out"), (dict(d_dists_out=None), ERR_ARG, "d_dists_out"), (dict(d_matched=None), ERR_ARG, "d_matched"),
]


def test_kernel_entry_refusals_before_any_hip_call(libbang):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    from bang_amd import binding as B
    fn = libbang.bang_k_scan
    fn.argtypes = [C.c_void_p, C.c_void_p]
    assert fn(None, None) == ERR_ARG and "bang_k_scan" in _err(libbang)
    for kw, code, word in _REFUSALS:
        p = B.ScanParams()
        for k, v in {**_GOOD, **kw}.items():
            setattr(p, k, v)
        assert fn(C.byref(p), None) == code, (kw, _err(libbang))
        assert word in _err(libbang) and "bang_k_scan" in _err(libbang), (kw, _err(libbang))
    libbang.bang_scan_check.argtypes = [C.c_void_p]
    p = B.ScanParams()
    for k, v in _GOOD.items():
        setattr(p, k, v)
    assert libbang.bang_scan_check(C.byref(p)) == OK
    libbang.bang_k_bitmap_or.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
    assert libbang.bang_k_bitmap_or(None, 0x1000, 4, 0, 0, None) == ERR_ARG and "d_dst" in _err(libbang)
    assert libbang.bang_k_bitmap_or(0x1000, None, 4, 0, 0, None) == ERR_ARG and "d_src" in _err(libbang)
    assert libbang.bang_k_bitmap_or(0x1000, 0x2000, 0, 0, 0, None) == OK       # no word: no launch, no HIP call


def test_geometry_through_ctypes(libbang):
    lib = libbang
    lib.bang_scan_geometry.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.bang_scan_max_stripes.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    lib.bang_scan_max_stripes.restype = C.c_uint32
    lib.bang_scan_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.bang_scan_scratch_bytes.restype = C.c_uint64
    t, s = C.c_uint32(0), C.c_uint32(0)
    for dtype, qt, rnd in ((0, 32, 128), (1, 32, 128), (2, 16, 256)):
        for n, nq, k in ((1, 1, 1), (4000, 64, 10), (4000, 130, 128), (1000000, 100, 10), (1000000, 4096, 100)):
            assert lib.bang_scan_geometry(dtype, 128, nq, n, k, C.byref(t), C.byref(s)) == OK
            most = lib.bang_scan_max_stripes(dtype, n, k)
            assert t.value == -(-nq // qt) and 1 <= s.value <= most == min(4096 // k, -(-n // rnd))
    assert lib.bang_scan_geometry(0, 128, 100, 1000000, 10, C.byref(t), C.byref(s)) == OK and s.value > 1      # few tiles: the points are striped
    assert lib.bang_scan_geometry(0, 48, 1, 10, 1, C.byref(t), C.byref(s)) == ERR_UNSUPPORTED
    assert lib.bang_scan_geometry(0, 128, 0, 10, 1, C.byref(t), C.byref(s)) == ERR_ARG
    assert lib.bang_scan_scratch_bytes(64, 10, 2) == 8 * 64 * 20 + 8 * 64


def test_host_side_under_sanitizers(tmp_path):
    """csrc/bang_scan_host.cpp + tests/scan_host_main.cpp built with -fsanitize=address,undefined and run: the geometry over a grid of shapes up
    to 2^32 - 1 nodes and 2^20 queries, and every refusal of the argument check."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scan_host_san")
    cmd = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "bang_scan_host.cpp"),
           os.path.join(ROOT, "tests", "scan_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) == 3 * 14 * 10 * 4 + 12 + 23


def test_kernels_use_no_private_segment(libbang, tmp_path):
    """The gfx950 code object of bang_scan.o: the ten scan8_kernel instances (uint8 / int8 x D = 16, 32, 64, 128, 256) and scan_f32_kernel with
    .private_segment_fixed_size == 0 and no spill, the i8 MFMA in the code, and not one flat_ / scratch_ instruction in the object."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_scan.o")
    assert all(os.path.exists(t) for t in tools), "llvm binutils are not here"
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        name = blk.split()[0]
        if "scan8_kernel" in name or "scan_f32_kernel" in name or "scan_out_kernel" in name or "bitmap_or_kernel" in name:
            found[name] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)))
    assert sum("scan8_kernel" in n for n in found) == 10 and sum("scan_f32_kernel" in n for n in found) == 1, sorted(found)
    assert all(v == (0, 0) for v in found.values()), found
    asm = subprocess.run([tools[3], "-d", co], check=True, capture_output=True, text=True).stdout
    assert "v_mfma_i32_32x32x32_i8" in asm and re.search(r"\bv_dot4c?_i32_i8", asm) and re.search(r"\bv_(pk_)?fmac?_f32", asm)
    assert not re.search(r"\b(flat|scratch)_\w+", asm)
