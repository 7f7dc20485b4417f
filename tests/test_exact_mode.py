"""Exact-distance search mode (option "distance" = 1) -- what can be checked without a GPU: the option, the exported kernel, its code object,
and the CPU reference composition the GPU tests compare against (tests/exact_reference.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from exact_reference import Reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distance_option_is_in_the_table_and_range_checked(libbang):
    lib = libbang
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    assert re.search(r"^  distance\s+BANG_DISTANCE\s+\[0, 1\]\s+bang_alloc\s", buf.value.decode(), flags=re.M)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == 0
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    try:
        assert lib.bang_set_option(h, b"distance", 0) == 0
        assert lib.bang_set_option(h, b"distance", 1) == 0
        assert lib.bang_set_option(h, b"distance", 2) != 0
        assert lib.bang_set_option(h, b"distance", -1) != 0
    finally:
        lib.bang_destroy.argtypes = [C.c_void_p]
        lib.bang_destroy(h)


def test_python_constants():
    import bang_amd
    assert (bang_amd.DISTANCE_PQ, bang_amd.DISTANCE_EXACT) == (0, 1)


def test_exact_kernel_is_declared_and_exported(libbang):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    for name in ("bang_k_search_exact", "bang_search_exact_geometry"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert hasattr(libbang, name), name
    assert re.search(r"int\s+bang_k_search_exact\s*\(\s*const\s+bang_search_params\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)


def test_exact_kernel_instances_run_without_scratch(libbang, tmp_path):
    """One instance per vector type (u8 / i8 / f32), no scratch -- read from the code object's kernel descriptors (ELF notes)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    obj = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_search_exact.o")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    assert os.path.exists(obj), obj
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", obj, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        m = re.match(r"_Z19search_exact_kernelILi(\d)EEv9ExactArgs$", blk.split()[0])
        if m:
            found[int(m.group(1))] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
    assert sorted(found) == [0, 1, 2], found
    assert all(v == 0 for v in found.values()), found


FIXTURES = ("small_u8", "small_f32", "small_i8", "small_deep")


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("L", [10, 37, 152])
def test_pq_composition_equals_the_oracle(name, L, request):
    """The composition in `pq` mode IS the oracle's search, bit for bit: ids, distance bits and per-query statistics."""
    from oracle import oracle as O
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:16]
    ids_o, d_o, st_o = O.Oracle(ix).search(q, 10, L, with_stats=True)
    ids, d, st = Reference(ix).search(q, 10, L, "pq")
    assert np.array_equal(ids, ids_o)
    assert np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
    assert np.array_equal(st, st_o)


@pytest.mark.parametrize("name", FIXTURES)
def test_exact_reference_is_self_consistent(name, request):
    from oracle import oracle as O
    ix, q, gt_i, gt_d = request.getfixturevalue(name)
    ref = Reference(ix)
    L = 37
    ids, d, st = ref.search(q, 10, L, "exact")
    for i in range(q.shape[0]):
        row = ids[i]
        ok = row != np.iinfo(np.uint64).max
        assert ok.all()                                                  # the worklist holds k entries at L >= k
        want = ref.exact(row.astype(np.uint32), np.ascontiguousarray(q[i], dtype=O.NP_DTYPE[ix.dtype]))
        assert np.array_equal(d[:, i].view(np.uint32), want.view(np.uint32))
        assert np.all(np.diff(d[:, i]) >= 0)
        assert len(set(row.tolist())) == len(row)
        assert st[i][1] >= 1 and st[i][0] <= L + 49
    rec_exact = O.recall(gt_i, gt_d, ids, 10)
    ids_pq, _, _ = ref.search(q, 10, L, "pq")
    rec_pq = O.recall(gt_i, gt_d, ids_pq, 10)
    print(f"{name}: 10-recall@10 at L = {L}: exact {rec_exact:.1f} %, pq + re-rank {rec_pq:.1f} %")
    assert rec_exact > 0.0
