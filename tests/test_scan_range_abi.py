"""The exact range scan's ABI without a GPU (csrc/bang_scan_range_host.cpp, no HIP call; DESIGN.md section 2 CANON 26): the exports exist, check and
entry refuse by name before any HIP call, the geometry keeps its bounds, the engine entry refuses on an empty handle and leaves its outputs alone,
and the cross-compiled kernels use no private segment."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
_GOOD = dict(d_vec_base=0x10000, vec_stride=100, dtype=1, D=100, n_nodes=4000, d_queries=0x20000, nq=64, d_radius=0x21000, max_hits=64, runs=3,
             d_scratch=0x30000, scratch_bytes=4 * 64 * 3, d_hit_ids=0x40000, d_hit_dists=0x50000, d_offered=0x60000, d_count=0x61000, d_matched=0x62000)
_CASES = [(dict(), OK, ""), (dict(dtype=2, D=1, vec_stride=4), OK, ""), (dict(dtype=0, D=1024, vec_stride=1024, max_hits=4096), OK, ""),
          (dict(runs=0, scratch_bytes=4 * 64 * 16), OK, ""), (dict(d_labels=0x70000, d_filters=0x71000), OK, "")]
_CASES += [({name: None}, ERR_ARG, name) for name in ("d_vec_base", "d_queries", "d_radius", "d_scratch", "d_hit_ids", "d_hit_dists", "d_offered",
                                                       "d_count", "d_matched")]
_CASES += [
    (dict(max_hits=0), ERR_ARG, "max_hits = 0"), (dict(max_hits=4097), ERR_ARG, "max_hits = 4097"), (dict(nq=0), ERR_ARG, "nq = 0"),
    (dict(n_nodes=0), ERR_ARG, "n_nodes"), (dict(D=0), ERR_UNSUPPORTED, "D = 0"), (dict(D=1028, vec_stride=1028), ERR_UNSUPPORTED, "D = 1028"),
    (dict(D=18, vec_stride=20), ERR_UNSUPPORTED, "D % 4 == 0"), (dict(dtype=3), ERR_UNSUPPORTED, "dtype"),
    (dict(vec_stride=96), ERR_UNSUPPORTED, "vec_stride"), (dict(vec_stride=102), ERR_UNSUPPORTED, "vec_stride"),
    (dict(d_labels=0x70000), ERR_ARG, "d_labels"), (dict(runs=126), ERR_ARG, "runs"),            # ceil(4000 / 32) = 125 tiles
    (dict(scratch_bytes=4 * 64 * 3 - 1), ERR_ARG, "scratch_bytes"), (dict(d_scratch=0x30004), ERR_ARG, "d_scratch"),
]


def _err(lib):
    lib.bang_last_error.restype = C.c_char_p
    return lib.bang_last_error().decode()


@pytest.mark.parametrize("kw,code,word", _CASES)
def test_check_and_entry_before_any_hip_call(libbang, kw, code, word):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    from bang_amd import binding as B
    p = B.ScanRangeParams()
    for k, v in {**_GOOD, **kw}.items():
        setattr(p, k, v)
    libbang.bang_scan_range_check.argtypes = [C.c_void_p]
    libbang.bang_k_scan_range.argtypes = [C.c_void_p, C.c_void_p]
    assert libbang.bang_scan_range_check(C.byref(p)) == code, (kw, _err(libbang))
    if code != OK:
        assert word in _err(libbang) and "bang_k_scan_range" in _err(libbang), (kw, _err(libbang))
        assert libbang.bang_k_scan_range(C.byref(p), None) == code and word in _err(libbang)


def test_geometry_and_scratch(libbang):
    lib = libbang
    lib.bang_scan_range_geometry.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bang_scan_range_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
    lib.bang_scan_range_scratch_bytes.restype = C.c_uint64
    t, r, m = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    for dtype, D, qt in ((0, 128, 32), (1, 100, 32), (2, 1, 16), (2, 1023, 16)):
        for n, nq in ((1, 1), (33, 1), (4000, 64), (1000000, 100), (1000000, 4096), (0xFFFFFFFF, 1 << 20)):
            assert lib.bang_scan_range_geometry(dtype, D, nq, n, C.byref(t), C.byref(r), C.byref(m)) == OK
            assert t.value == -(-nq // qt) and 1 <= r.value <= m.value <= min(-(-n // 32), 4096)
            assert 4 * nq * m.value <= max(64 << 20, 4 * nq), "the counts of the largest launch pass 64 MB"
    assert lib.bang_scan_range_geometry(0, 128, 100, 1000000, C.byref(t), C.byref(r), None) == OK and r.value * t.value >= 2048      # fills the chip
    assert lib.bang_scan_range_geometry(0, 18, 1, 10, C.byref(t), C.byref(r), None) == ERR_UNSUPPORTED
    assert lib.bang_scan_range_geometry(2, 1025, 1, 10, C.byref(t), C.byref(r), None) == ERR_UNSUPPORTED
    assert lib.bang_scan_range_geometry(0, 128, 0, 10, C.byref(t), C.byref(r), None) == ERR_ARG
    assert lib.bang_scan_range_geometry(0, 128, 1, 0, C.byref(t), C.byref(r), None) == ERR_ARG
    assert lib.bang_scan_range_scratch_bytes(64, 3) == 4 * 64 * 3


def test_engine_entry_on_an_empty_handle(libbang):
    lib = libbang
    from bang_amd import binding as B
    assert callable(B.Engine.scan_range) and callable(B.Engine.scan_range_times)
    lib.bang_scan_range_e.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    q, rad = np.zeros((4, 128), np.uint8), np.ones(4, np.float32)
    ids, dists = np.full((4, 8), 7, np.uint64), np.full((4, 8), 7.0, np.float32)
    words = [np.full(4, 7, np.uint32) for _ in range(3)]
    out = [a.ctypes.data for a in (ids, dists, *words)]
    assert lib.bang_scan_range_e(None, q.ctypes.data, 4, rad.ctypes.data, 8, None, None, *out) == ERR_ARG and "bang_scan_range" in _err(lib)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    for nq, hits in ((4, 8), (0, 8), (4, 0), (4, 4097)):          # nothing is loaded: said first, whatever else is wrong with the call
        assert lib.bang_scan_range_e(h, q.ctypes.data, nq, rad.ctypes.data, hits, None, None, *out) == ERR_ARG
        assert "bang_scan_range" in _err(lib) and "no index is loaded" in _err(lib)
    assert (ids == 7).all() and (dists == 7.0).all() and all((w == 7).all() for w in words), "a refused call wrote an output buffer"
    lib.bang_get_scan_range_times.argtypes = [C.c_void_p, C.c_void_p]
    ms = (C.c_double * 2)(1, 1)
    assert lib.bang_get_scan_range_times(h, None) == ERR_ARG and lib.bang_get_scan_range_times(h, ms) == OK and list(ms) == [0, 0]
    lib.bang_destroy.argtypes = [C.c_void_p]
    lib.bang_destroy(h)


def test_kernels_use_no_private_segment(libbang, tmp_path):
    """The gfx950 code object of bang_scan_range.o, from its ELF notes: the four scan_range8_kernel instances (uint8 / int8 x count / emit), the two
    scan_range_f32_kernel instances and the prefix kernel with .private_segment_fixed_size == 0 and no register spilled to memory."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    path = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_scan_range.o")
    assert all(os.path.exists(t) for t in tools), "llvm binutils are not here"
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", path, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        found[blk.split()[0]] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1)))
    count = lambda word: sum(word in n for n in found)      # noqa: E731
    assert (count("scan_range8_kernel"), count("scan_range_f32_kernel"), count("scan_range_prefix_kernel")) == (4, 2, 1) and len(found) == 7, sorted(found)
    assert all(v == (0, 0) for v in found.values()), found
