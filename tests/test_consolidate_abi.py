"""The consolidation ABI without a GPU: the exports exist, bang_stats_ext6 extends ext5 without moving a member, every refusal that needs no device
comes with its code and message before any HIP call, the test hook lives in the environment table, and the host-side listing
(csrc/bang_consolidate_group.cpp, no HIP call) is built with a stand-alone main under -fsanitize=address,undefined and run as a program (no Python
runs under a sanitizer)."""
import ctypes as C
import os
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
    for sym in ("bang_consolidate_e", "bang_get_stats_ext6", "bang_get_consolidate_times", "bang_k_consolidate_scan", "bang_k_consolidate_gather",
                "bang_k_consolidate_clear", "bang_consolidate_group"):
        getattr(libbang, sym)


def test_stats_ext6_extends_ext5_without_moving_a_member():
    from bang_amd import binding as B
    assert B.StatsExt6._fields_[:len(B.StatsExt5._fields_)] == B.StatsExt5._fields_
    assert C.sizeof(B.StatsExt6) == C.sizeof(B.StatsExt5) + 3 * 8
    assert [f for f, _ in B.StatsExt6._fields_[-3:]] == ["consolidated_rows", "removed", "consolidate_dropped"]
    assert all(t is C.c_uint64 for _, t in B.StatsExt6._fields_[-3:])


def test_the_chunk_hook_is_in_the_environment_table(libbang):
    lib = libbang
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    assert "BANG_CONSOLIDATE_CHUNK" in buf.value.decode()


def test_engine_refusals_that_need_no_device(libbang):
    from bang_amd import binding as B
    lib = libbang
    lib.bang_consolidate_e.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    st = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert lib.bang_consolidate_e(None, 1.2, st) == ERR_ARG and "bang_consolidate" in _err(lib) and "null" in _err(lib)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    assert lib.bang_set_option(h, b"capacity", 5000) == OK
    for alpha in (1.2, float("nan")):                                      # nothing is loaded: said first, whatever alpha is
        assert lib.bang_consolidate_e(h, alpha, st) == ERR_ARG and "bang_consolidate" in _err(lib) and "no index is loaded" in _err(lib)
    assert list(st) == [7, 7, 7, 7], "a refused call wrote its statistics"
    lib.bang_get_stats_ext6.argtypes = [C.c_void_p, C.c_void_p]
    lib.bang_get_consolidate_times.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.bang_get_stats_ext6(h, None) == ERR_ARG and lib.bang_get_stats_ext6(None, None) == ERR_ARG
    s = B.StatsExt6()
    assert lib.bang_get_stats_ext6(h, C.byref(s)) == OK
    assert (s.capacity, s.consolidated_rows, s.removed, s.consolidate_dropped) == (5000, 0, 0, 0)
    ms = (C.c_double * 4)(1, 1, 1, 1)
    assert lib.bang_get_consolidate_times(h, None) == ERR_ARG and lib.bang_get_consolidate_times(h, ms) == OK and list(ms) == [0, 0, 0, 0]
    lib.bang_destroy.argtypes = [C.c_void_p]
    lib.bang_destroy(h)


_TABLE = dict(d_graph=0x1000, entry_len=128 + 4 + 4 * 64, dtype=0, D=128, R=64, n_nodes=100, medoid=3, d_excluded=0x2000)


def _params(entry, **kw):
    from bang_amd import binding as B
    cls, extra = {"scan": (B.ConsolidateScanParams, dict(d_affected=0x3000)),
                  "gather": (B.ConsolidateGatherParams, dict(n_lists=3, d_nodes=0x3000, d_cand_ids=0x4000, d_cand_dists=0x5000, d_offered=0x6000,
                                                             d_own_out=0x7000, d_stats=0x8000)),
                  "clear": (B.ConsolidateClearParams, {})}[entry]
    p = cls()
    for k, v in {**_TABLE, **extra, **kw}.items():
        setattr(p, k, v)
    return p


_COMMON = [
    (dict(d_graph=None), ERR_ARG, "d_graph"), (dict(d_graph=0x1002), ERR_ARG, "d_graph"), (dict(d_excluded=None), ERR_ARG, "d_excluded"),
    (dict(R=0), ERR_ARG, "R = 0"), (dict(R=65), ERR_ARG, "R = 65"), (dict(n_nodes=0), ERR_ARG, "n_nodes"), (dict(medoid=100), ERR_ARG, "medoid"),
    (dict(D=48, entry_len=48 + 4 + 256), ERR_UNSUPPORTED, "layout"),      # 8-bit D / 16 = 3: a wide layout
    (dict(D=320, dtype=2, entry_len=4 * 320 + 260), ERR_UNSUPPORTED, "layout"),
    (dict(entry_len=128 + 4 * 64), ERR_UNSUPPORTED, "layout"),            # the entry stride does not hold vector and row
    (dict(dtype=3), ERR_UNSUPPORTED, "layout"),
]
_OWN = {"scan": [(dict(d_affected=None), ERR_ARG, "d_affected")],
        "gather": [(dict(d_nodes=None), ERR_ARG, "d_nodes"), (dict(d_cand_ids=None), ERR_ARG, "d_cand_ids"), (dict(d_cand_dists=None), ERR_ARG, "d_cand_dists"),
                   (dict(d_offered=None), ERR_ARG, "d_offered"), (dict(d_own_out=None), ERR_ARG, "d_own_out"), (dict(d_stats=None), ERR_ARG, "d_stats")],
        "clear": []}


@pytest.mark.parametrize("entry", ["scan", "gather", "clear"])
def test_kernel_entry_refusals_before_any_hip_call(libbang, entry):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    fn = getattr(libbang, "bang_k_consolidate_" + entry)
    fn.argtypes = [C.c_void_p, C.c_void_p]
    assert fn(None, None) == ERR_ARG and "bang_k_consolidate_" + entry in _err(libbang)
    for kw, code, word in _COMMON + _OWN[entry]:
        assert fn(C.byref(_params(entry, **kw)), None) == code, (kw, _err(libbang))
        assert word in _err(libbang) and "bang_k_consolidate_" + entry in _err(libbang), (kw, _err(libbang))
    if entry == "gather":
        assert fn(C.byref(_params(entry, n_lists=0)), None) == OK              # no list: no launch, no HIP call


def test_group_through_ctypes(libbang):
    lib = libbang
    lib.bang_consolidate_group.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    for n, ids in ((0, []), (1, [0]), (31, [0, 30]), (32, [31]), (33, [0, 31, 32]), (130, [0, 63, 64, 127, 128, 129]), (130, list(range(130))), (130, [])):
        bits = np.zeros((n + 31) // 32 + 1, np.uint32)
        for x in ids:
            bits[x >> 5] |= np.uint32(1 << (x & 31))
        if n % 32:
            bits[n // 32] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)      # bits behind n belong to no node
        bits[-1] = 0xFFFFFFFF                                                       # ... and neither does the slack word
        out = np.full(max(n, 1), 0xEEEEEEEE, np.uint32)
        cnt = C.c_uint32(99)
        assert lib.bang_consolidate_group(bits.ctypes.data, n, out.ctypes.data, C.byref(cnt)) == OK
        assert cnt.value == len(ids) and list(out[:cnt.value]) == ids, (n, ids)
        assert (out[cnt.value:] == 0xEEEEEEEE).all()
    assert lib.bang_consolidate_group(None, 4, out.ctypes.data, C.byref(cnt)) == ERR_ARG


def test_group_under_sanitizers(tmp_path):
    """csrc/bang_consolidate_group.cpp + tests/consolidate_group_main.cpp built with -fsanitize=address,undefined and run: bitmaps of 0, 1, 31, 32,
    33 and 130 nodes, all set, none set and random, with the slack bits of the last word set; every array heap-allocated to the size the contract
    names."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "consolidate_group_san")
    cmd = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "bang_consolidate_group.cpp"),
           os.path.join(ROOT, "tests", "consolidate_group_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) == 36
