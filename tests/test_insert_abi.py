"""The insert ABI without a GPU: the exports exist, every refusal that needs no device comes with its code and message before any HIP call, option
capacity lives in the option table, and the host-side grouping (csrc/bang_insert_group.cpp, no HIP call) is built with a stand-alone main under
-fsanitize=address,undefined and run as a program (no Python runs under a sanitizer)."""
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
    for sym in ("bang_insert_e", "bang_get_entries_e", "bang_get_codes_e", "bang_get_stats_ext5", "bang_k_prune", "bang_k_worklist_lists",
                "bang_k_backedge", "bang_k_pq_encode", "bang_insert_group"):
        getattr(libbang, sym)


def test_stats_ext5_extends_ext4_without_moving_a_member():
    from bang_amd import binding as B
    assert B.StatsExt5._fields_[:len(B.StatsExt4._fields_)] == B.StatsExt4._fields_
    assert C.sizeof(B.StatsExt5) == C.sizeof(B.StatsExt4) + 5 * 8
    assert [f for f, _ in B.StatsExt5._fields_[-5:]] == ["capacity", "inserted", "backedge_appended", "backedge_pruned", "backedge_dropped"]


def test_option_capacity(libbang):
    lib = libbang
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    assert "  capacity " in buf.value.decode() and "BANG_CAPACITY" in buf.value.decode()
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    assert lib.bang_set_option(h, b"capacity", 0) == OK and lib.bang_set_option(h, b"capacity", 5000) == OK
    for bad in (-1, 0xFFFFFFFF, 1 << 40):                                 # >= 0xFFFFFFFF never reaches a load
        assert lib.bang_set_option(h, b"capacity", bad) == ERR_ARG and "capacity" in _err(lib)
    lib.bang_destroy.argtypes = [C.c_void_p]
    lib.bang_destroy(h)


def test_engine_refusals_that_need_no_device(libbang):
    lib = libbang
    lib.bang_insert_e.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    lib.bang_get_entries_e.argtypes = lib.bang_get_codes_e.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    v = np.zeros((4, 128), np.uint8)
    first = C.c_uint64(77)
    assert lib.bang_insert_e(None, v.ctypes.data, 4, 32, 1.2, C.byref(first)) == ERR_ARG and "null" in _err(lib)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    assert lib.bang_set_option(h, b"capacity", 5000) == OK
    assert lib.bang_insert_e(h, v.ctypes.data, 4, 32, 1.2, C.byref(first)) == ERR_ARG and "no index is loaded" in _err(lib)
    assert first.value == 77
    out = np.zeros(16, np.uint8)
    assert lib.bang_get_entries_e(h, 0, 1, out.ctypes.data) == ERR_ARG and "bang_get_entries" in _err(lib)
    assert lib.bang_get_codes_e(h, 0, 1, out.ctypes.data) == ERR_ARG and "bang_get_codes" in _err(lib)
    assert lib.bang_get_stats_ext5(h, None) == ERR_ARG
    from bang_amd import binding as B
    s = B.StatsExt5()
    assert lib.bang_get_stats_ext5(h, C.byref(s)) == OK and s.capacity == 5000 and s.inserted == 0
    lib.bang_destroy.argtypes = [C.c_void_p]
    lib.bang_destroy(h)


def test_capacity_is_refused_by_streamed_and_shared_loads_before_any_hip_call(libbang):
    """bang_load_stream_e / bang_load_shared_e (the loads that take a caller's vector buffer, bang_index_desc.d_vectors) with option capacity set:
    BANG_ERR_UNSUPPORTED with "capacity" in the message, in front of the device check -- every pointer of the descriptor is a made-up address and
    the entry source is never called."""
    from bang_amd import binding as B
    lib = libbang
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.bang_load_stream_e.argtypes = [C.c_void_p, C.c_void_p, B.ENTRY_SOURCE, C.c_void_p]
    lib.bang_load_shared_e.argtypes = [C.c_void_p, C.c_void_p]
    lib.bang_destroy.argtypes = [C.c_void_p]
    called = []
    src = B.ENTRY_SOURCE(lambda ctx, first, count, dst: called.append(first) or 1)
    D, R, N, m = 128, 64, 1000, 32
    for d_vectors in (None, 0x7000):
        d = B.IndexDesc(0, D + 4 + 4 * R, D, R, N, m, None, 0x1000, None, 0x2000, 0x3000, 0x4000, 0, 0, d_vectors, 0)
        h = C.c_void_p()
        assert lib.bang_create(0, C.byref(h)) == OK
        assert lib.bang_set_option(h, b"capacity", 2 * N) == OK
        assert lib.bang_load_stream_e(h, C.byref(d), src, None) == ERR_UNSUPPORTED
        assert "capacity" in _err(lib) and "streamed" in _err(lib)
        lib.bang_destroy(h)
    d = B.IndexDesc(0, D + 4 + 4 * R, D, R, N, m, None, 0x1000, None, 0x2000, 0x3000, 0x4000, 0, 1, 0x7000, 5)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == OK
    assert lib.bang_set_option(h, b"capacity", 2 * N) == OK
    assert lib.bang_load_shared_e(h, C.byref(d)) == ERR_UNSUPPORTED
    assert "capacity" in _err(lib) and "shared" in _err(lib)
    lib.bang_destroy(h)
    assert not called


def _prune_params(**kw):
    from bang_amd import binding as B
    p = B.PruneParams()
    good = dict(d_graph=0x1000, entry_len=128 + 4 + 4 * 64, dtype=B.U8, D=128, n_nodes=100, R=64, alpha2=1.44, n_lists=3, list_stride=64,
                d_list_ids=0x2000, d_list_dists=0x3000, d_list_cnt=0x4000, d_own=0x5000, d_out=0x6000, out_stride=4 * 65, out_by_own=0)
    good.update(kw)
    for k, v in good.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, code, word", [
    (dict(d_graph=None), ERR_ARG, "d_graph"), (dict(d_graph=0x1002), ERR_ARG, "d_graph"),
    (dict(d_list_ids=None), ERR_ARG, "d_list_ids"), (dict(d_list_dists=None), ERR_ARG, "d_list_dists"), (dict(d_list_cnt=None), ERR_ARG, "d_list_cnt"),
    (dict(d_own=None), ERR_ARG, "d_own"), (dict(d_out=None), ERR_ARG, "d_out"),
    (dict(R=0), ERR_ARG, "R = 0"), (dict(R=65), ERR_ARG, "R = 65"), (dict(list_stride=0), ERR_ARG, "list_stride"),
    (dict(out_stride=4 * 64), ERR_ARG, "out_stride"), (dict(out_stride=4 * 65 + 2), ERR_ARG, "out_stride"),
    (dict(n_nodes=0), ERR_ARG, "n_nodes"),
    (dict(alpha2=0.99), ERR_ARG, "alpha2"), (dict(alpha2=64.5), ERR_ARG, "alpha2"), (dict(alpha2=float("nan")), ERR_ARG, "alpha2"),
    (dict(D=48, entry_len=48 + 4 + 256), ERR_UNSUPPORTED, "layout"),     # 8-bit D / 16 = 3: a wide layout
    (dict(D=320, dtype=2, entry_len=4 * 320 + 260), ERR_UNSUPPORTED, "layout"),
    (dict(D=128, entry_len=390), ERR_UNSUPPORTED, "layout"),
    (dict(dtype=3), ERR_UNSUPPORTED, "layout"),
])
def test_prune_refusals_before_any_hip_call(libbang, kw, code, word):
    """(every pointer here is a made-up address: a launch, or any HIP call that touched one, could not return these codes)"""
    lib = libbang
    lib.bang_k_prune.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.bang_k_prune(C.byref(_prune_params(**kw)), None) == code
    assert word in _err(lib), _err(lib)


def test_prune_null_params_and_empty_launch(libbang):
    lib = libbang
    lib.bang_k_prune.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.bang_k_prune(None, None) == ERR_ARG
    assert lib.bang_k_prune(C.byref(_prune_params(n_lists=0)), None) == OK        # no list: no launch, no HIP call


def test_encode_lists_and_backedge_refusals(libbang):
    lib = libbang
    lib.bang_k_pq_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_uint64, C.c_void_p]
    good = [0x1000, 0x2000, 0, 0x3000, 0x4000, 0x5000, 8, 4, 128, 70, 0x6000, 70, None]
    for at, val, word in ((0, None, "d_pivots_T"), (1, None, "d_vectors"), (3, None, "d_centroid"), (4, None, "d_chunk_off"), (5, None, "d_lut"),
                          (10, None, "d_codes"), (2, 3, "dtype"), (9, 0, "m = 0"), (9, 129, "m = 129"), (6, 0, "lut_points"), (11, 69, "code_stride")):
        a = list(good)
        a[at] = val
        assert lib.bang_k_pq_encode(*a) == ERR_ARG and word in _err(lib), (at, _err(lib))
    a = list(good)
    a[7] = 0
    assert lib.bang_k_pq_encode(*a) == OK                                  # n = 0: nothing to do
    lib.bang_k_worklist_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                          C.c_void_p, C.c_void_p]
    good = [0x1000, 0x2000, 40, 0, 4, 4, 0x3000, 0x4000, 40, 0x5000, None]
    for at, val, word in ((0, None, "d_wl_ids"), (1, None, "d_wl_dists"), (6, None, "d_list_ids"), (7, None, "d_list_dists"), (9, None, "d_list_cnt"),
                          (2, 0, "L = 0"), (2, 513, "L = 513"), (8, 39, "list_stride"), (5, 3, "Q_total")):
        a = list(good)
        a[at] = val
        assert lib.bang_k_worklist_lists(*a) == ERR_ARG and word in _err(lib), (at, _err(lib))
    lib.bang_k_backedge.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.bang_k_backedge(None, None) == ERR_ARG


def test_group_through_ctypes(libbang):
    lib = libbang
    lib.bang_insert_group.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 4
    rows = np.array([[2, 7, 3, 0], [3, 3, 9, 7], [0, 0, 0, 0], [1, 3, 0, 0]], np.uint32)
    n, R = 4, 3
    t, o, s = np.zeros(n * R, np.uint32), np.zeros(n * R + 1, np.uint32), np.zeros(n * R, np.uint32)
    nt = C.c_uint32(0)
    assert lib.bang_insert_group(rows.ctypes.data, n, R + 1, 100, 10, t.ctypes.data, o.ctypes.data, s.ctypes.data, C.byref(nt)) == OK
    assert nt.value == 3 and list(t[:3]) == [3, 7, 9] and list(o[:4]) == [0, 3, 5, 6] and list(s[:6]) == [100, 101, 103, 100, 101, 101]
    assert lib.bang_insert_group(rows.ctypes.data, n, R + 1, 100, 9, t.ctypes.data, o.ctypes.data, s.ctypes.data, C.byref(nt)) == ERR_ARG   # id 9 >= n_old


def test_group_under_sanitizers(tmp_path):
    """csrc/bang_insert_group.cpp + tests/insert_group_main.cpp built with -fsanitize=address,undefined and run: random batches up to 1000 rows of
    64 ids, every array heap-allocated to the size the contract names."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "insert_group_san")
    cmd = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "bang_insert_group.cpp"),
           os.path.join(ROOT, "tests", "insert_group_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) >= 60
