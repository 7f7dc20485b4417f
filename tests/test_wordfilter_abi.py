"""C-ABI of the word-local visited filter (option "filter_layout"), without a GPU: the exports, the option table, the statistics field and
the refusals bang_k_search_wf makes BEFORE any HIP call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
EXPORTS = ("bang_k_search_wf", "bang_search_wf_geometry", "bang_search_wf_has_instance", "bang_get_stats_ext")
KEYS = (108, 116, 124, 132, 208, 216, 218, 219, 404, 408, 802, 804)          # BANG_PQ_LAYOUTS, csrc/bang_search_args.h


def _options(lib):
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    return buf.value.decode()


def test_the_three_exports_exist_and_are_declared(libbang):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    for name in EXPORTS:
        assert hasattr(libbang, name), name
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M), name


def test_filter_layout_is_in_the_option_table_and_range_checked(libbang):
    lib = libbang
    text = _options(lib)
    assert re.search(r"^  filter_layout\s+BANG_FILTER_LAYOUT\s+\[0, 1\]\s+bang_alloc\s", text, flags=re.M)
    line = [l for l in text.splitlines() if l.strip().startswith("filter_layout ")]
    assert len(line) == 1 and "(environment: split | word)" in line[0] and not line[0].rstrip().endswith(('"', ",")), line
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == 0
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    try:
        assert lib.bang_set_option(h, b"filter_layout", 0) == OK
        assert lib.bang_set_option(h, b"filter_layout", 1) == OK
        assert lib.bang_set_option(h, b"filter_layout", 2) == ERR_ARG
        assert lib.bang_set_option(h, b"filter_layout", -1) == ERR_ARG
    finally:
        lib.bang_destroy.argtypes = [C.c_void_p]
        lib.bang_destroy(h)


def test_environment_words_are_parsed_through_the_table():
    src = open(os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_options.cpp")).read()
    body = src[src.index("void apply_env_defaults"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"&bang_engine::filter_layout.*\n\s*x = strcmp\(v, \"word\"\) == 0 \? 1 : 0;", body), body


def test_extended_stats_struct_carries_the_field(libbang, tmp_path):
    """bang_stats keeps its size and members (tests/test_vectors_fp16_abi.py pins its last one); filter_layout is appended behind it in
    bang_stats_ext, which bang_get_stats_ext fills and Engine.stats() reads.  Header and ctypes mirror agree (a C program prints the layout)."""
    import shutil
    import subprocess
    from bang_amd import binding as B
    assert hasattr(libbang, "bang_get_stats_ext")
    assert B.StatsExt._fields_[:-1] == B.Stats._fields_ and B.StatsExt._fields_[-1] == ("filter_layout", C.c_uint64)
    assert C.sizeof(B.StatsExt) == C.sizeof(B.Stats) + 8 and B.StatsExt.filter_layout.offset == C.sizeof(B.Stats)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*bang_stats base;\s*uint64_t filter_layout;\s*\}\s*bang_stats_ext;", hdr)
    assert re.search(r"^int\s+bang_get_stats_ext\s*\(", hdr, flags=re.M)
    assert libbang.bang_get_stats_ext(None, None) == ERR_ARG
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc:
        c = tmp_path / "layout.c"
        c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bang_c.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(bang_stats), '
                     'sizeof(bang_stats_ext), offsetof(bang_stats_ext, filter_layout)); return 0; }\n')
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(c)])
        got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
        assert got == [C.sizeof(B.Stats), C.sizeof(B.StatsExt), B.StatsExt.filter_layout.offset]


def test_python_constants_and_entry():
    import bang_amd
    assert (bang_amd.FILTER_SPLIT, bang_amd.FILTER_WORD) == (0, 1)
    assert callable(bang_amd.IterState.run_search_wf)


def test_has_instance_follows_the_dispatch(libbang):
    f = libbang.bang_search_wf_has_instance
    f.argtypes = [C.c_uint32] * 3
    for key in KEYS:
        psz, mp = key // 100, 4 * (key % 100)
        assert f(psz, mp, mp) == 1 and f(psz, mp, mp - 1) == 1, key        # rows dword-aligned or not
    for psz, mp in ((0, 64), (2, 48), (4, 64), (8, 32), (1, 130), (3, 32)):
        assert f(psz, mp, mp) == 0, (psz, mp)


def test_every_layout_the_engine_can_choose_has_an_instance(libbang):
    """bang_alloc refuses filter_layout = 1 on a pivot layout without an instance -- and bang_pq_layout, which chooses the layout at load, only
    ever names layouts of search_dispatch (or the LUT path, psz 0, refused by its own message): that refusal guards a case no index reaches
    today, which is why no GPU test can provoke it."""
    import numpy as np
    from bang_amd import binding as B
    f = libbang.bang_search_wf_has_instance
    f.argtypes = [C.c_uint32] * 3
    seen = set()
    for width in (1, 2, 3, 4, 7, 8):
        for m in range(1, 129):
            psz, mp = B.pq_layout(np.arange(m + 1, dtype=np.uint32) * width, m * width, m)
            if psz:
                seen.add(psz * 100 + mp // 4)
                assert f(psz, mp, m) == 1, (width, m, psz, mp)
    assert seen == set(KEYS)


def test_geometry_is_that_of_the_self_paced_form(libbang):
    u32 = C.c_uint32
    out = []
    for name, extra in (("bang_search_wf_geometry", ()), ("bang_search_inmem_geometry", ())):
        g, w = u32(0), u32(0)
        rc = getattr(libbang, name)(u32(2), u32(72), u32(58), u32(37), u32(1), u32(0), u32(0), C.byref(g), C.byref(w))
        out.append((rc, g.value, w.value))
    assert out[0] == out[1] and out[0][0] == OK and out[0][1] == 1 and out[0][2] == 1


def _params(B, **over):
    """Arguments that pass every host-side check of search_setup (the pointers are never dereferenced on the host)."""
    sp = B.SearchParams()
    sp.Q, sp.R, sp.m, sp.L, sp.medoid, sp.cap_iter = 4, 32, 8, 37, 0, 37 + 49
    sp.psz, sp.mp = 4, 16
    sp.entry_len, sp.vec_bytes = 32 + 4 * 33, 32
    for f in ("d_seed", "d_codes", "d_pivots_packed", "d_qc", "d_graph", "d_bloom", "d_cand_ids", "d_cand_cnt", "d_next_query"):
        setattr(sp, f, 0x1000)
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


@pytest.mark.parametrize("over,code,message", [
    (dict(d_graph=None), ERR_UNSUPPORTED, "filter_layout = 1"),            # no host-paced instances
    (dict(d_bloom=None), ERR_ARG, "null buffer"),
    (dict(psz=0), ERR_UNSUPPORTED, "LDS-resident pivot layout"),
    (dict(cap_iter=37 + 50), ERR_ARG, "bad iteration cap"),
    (dict(L=0), ERR_ARG, "bad R/L/m"),
])
def test_launcher_refuses_before_any_hip_call(libbang, over, code, message):
    from bang_amd import binding as B
    libbang.bang_last_error.restype = C.c_char_p
    sp = _params(B, **over)
    assert libbang.bang_k_search_wf(C.byref(sp), None) == code
    assert message in libbang.bang_last_error().decode()
    assert libbang.bang_k_search_wf(None, None) == ERR_ARG
    sp = _params(B, Q=0)
    assert libbang.bang_k_search_wf(C.byref(sp), None) == OK               # an empty batch launches nothing


def test_documents_name_the_option():
    for doc, words in (("README.md", ("filter_layout", "BANG_FILTER_LAYOUT")), ("DESIGN.md", ("4.11", "filter_layout", "CANON 16")),
                       ("INTEGRATION.md", ("BANG_FILTER_LAYOUT",)), ("profiles/filter_layout.md", ("__hip_cuid", "VGPR"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
