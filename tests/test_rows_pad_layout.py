"""Adjacency rows in the padding of the PQ code table (option "rows_pad"), without a GPU.

* The layout (csrc/bang_pad_rows.h) and the launch checks on bang_search_params.n_rows_pad (csrc/bang_search_host.cpp): tests/pad_rows_layout_main.cpp,
  a program with its own main, built by the package Makefile's target pad_rows_layout_test -- plain, and with -fsanitize=address,undefined -- and run.
  No Python runs under a sanitizer.
* The option: its row of the option table, its range and its phase; the new member took padding of bang_search_params (no member moved); the
  launch check through the library itself.  What a load and an allocation resolve (auto on, auto given up, forced refused, the environment preset)
  needs a device: tests/test_gpu_rows_pad.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bang-billion-scale-ann_amd")
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
SANITIZE = "-fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -static-libasan -static-libubsan"


@pytest.mark.parametrize("flags", ["", SANITIZE], ids=["plain", "sanitized"])
def test_layout_program(tmp_path, flags):
    assert shutil.which("make") and (shutil.which("g++") or shutil.which("c++"))
    out = str(tmp_path / "bin")
    cmd = ["make", "-C", PKG, "-s", "pad_rows_layout_test", "PAD_TEST_OUT=" + out, "PAD_TEST_FLAGS=" + flags]
    if not shutil.which("g++"):
        cmd.append("HOSTCXX=c++")
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(out, "pad_rows_layout_test")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    # 4 usable layouts x (N = 4 | 5 | 6 | 1003 have padded rows) x 64 slots x 4 checks, and the rest
    assert m and int(m.group(1)) > 250_000, r.stdout


def _options(lib):
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    return buf.value.decode()


def test_option_row_range_and_phase(libbang):
    lib = libbang
    text = _options(lib)
    assert re.search(r"^  rows_pad\s+BANG_ROWS_PAD\s+\[-1, 1\]\s+bang_load\s", text, flags=re.M)
    line = [l for l in text.splitlines() if l.strip().startswith("rows_pad ")]
    assert len(line) == 1 and "-1 = auto" in line[0] and "1 = forced" in line[0] and "WRITTEN" in line[0], line
    assert line[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    lib.bang_destroy.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == 0
    try:
        for v, rc in ((-1, OK), (0, OK), (1, OK), (2, ERR_ARG), (-2, ERR_ARG)):
            assert lib.bang_set_option(h, b"rows_pad", v) == rc, v
        n = C.c_uint64(7)
        lib.bang_rows_pad_e.argtypes = [C.c_void_p, C.c_void_p]
        assert lib.bang_rows_pad_e(h, C.byref(n)) == OK and n.value == 0          # nothing loaded: no padded rows
        assert lib.bang_rows_pad_e(None, C.byref(n)) == ERR_ARG and lib.bang_rows_pad_e(h, None) == ERR_ARG
    finally:
        lib.bang_destroy(h)


def test_member_took_padding_and_header_agrees(libbang, tmp_path):
    from bang_amd import binding as B
    names = [f for f, _ in B.SearchParams._fields_]
    assert names[names.index("spec_rows") + 1] == "n_rows_pad" and names[names.index("n_rows_pad") + 1] == "rr_queries" and names[-1] == "d_lut"
    assert B.SearchParams.n_rows_pad.offset == B.SearchParams.spec_rows.offset + 4 and B.SearchParams.rr_queries.offset == B.SearchParams.n_rows_pad.offset + 4
    assert C.sizeof(B.SearchParams) == 376
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bang_c.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(bang_search_params), '
                 'offsetof(bang_search_params, spec_rows), offsetof(bang_search_params, n_rows_pad), offsetof(bang_search_params, rr_queries)); return 0; }\n')
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(c)])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    assert got == [376, B.SearchParams.spec_rows.offset, B.SearchParams.n_rows_pad.offset, B.SearchParams.rr_queries.offset]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"^int\s+bang_rows_pad_e\s*\(", hdr, flags=re.M)


def _params(B, **over):
    """a pulled-rows launch of the 70-chunk layout that passes every host-side check (the pointers are never dereferenced on the host)"""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.m, sp.L, sp.medoid, sp.cap_iter = 4, 64, 70, 37, 0, 37 + 49
    sp.psz, sp.mp, sp.pq_nhi, sp.code_stride = 2, 72, 58, 128
    sp.entry_len, sp.row_layout, sp.n_nodes = 256, 1, 1003
    for f in ("d_seed", "d_codes", "d_pivots_packed", "d_qc", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query"):
        setattr(sp, f, 0x1000)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


@pytest.mark.parametrize("entry,over,word", [
    ("bang_k_search", dict(n_rows_pad=201), "exceeds"),                         # row 200 would end behind line 1002
    ("bang_k_search", dict(n_rows_pad=200, n_nodes=999), "exceeds"),
    ("bang_k_search", dict(n_rows_pad=200, row_layout=0, entry_len=388, vec_bytes=128), "row_layout"),
    ("bang_k_search", dict(n_rows_pad=200, n_slices=2, slice_rows=512, d_row_slices=0x1000), "peer rows"),
    ("bang_k_search", dict(n_rows_pad=200, code_stride=0), "code_stride"),
    ("bang_k_search", dict(n_rows_pad=200, code_stride=256), "code_stride"),
    ("bang_k_search", dict(n_rows_pad=200, m=74, mp=76, pq_nhi=22), "PQ layout"),
    ("bang_k_search", dict(n_rows_pad=6, m=32, mp=32, psz=4, pq_nhi=0, code_stride=32), "PQ layout"),
    ("bang_k_search_wf", dict(n_rows_pad=200, m=74, mp=76, pq_nhi=22), "PQ layout"),
    ("bang_k_search", dict(n_rows_pad=200, d_graph=None, d_rows=0x1000, d_ctl=0x1000, h_done=0x1000, h_parents=0x1000), "host-paced"),
])
def test_launch_refuses_padded_rows_it_cannot_read_before_any_hip_call(libbang, entry, over, word):
    from bang_amd import binding as B
    libbang.bang_last_error.restype = C.c_char_p
    sp = _params(B, **over)
    assert getattr(libbang, entry)(C.byref(sp), None) == ERR_ARG
    msg = libbang.bang_last_error().decode()
    assert "n_rows_pad" in msg and "rows_pad" in msg and word in msg, msg
