"""The wide layouts of the exact-distance search mode (D up to 1024, 8-bit vectors with any D / 16) -- what can be checked without a GPU: the
inputs of tests/highdim_inputs.py reach their ground on the CPU reference, the layout predicate, and the new instances' code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import exact_reference as X
import highdim_inputs as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Recording(X.Reference):
    """The reference with every evaluated (ids, query) pair kept."""
    def __init__(self, ix):
        super().__init__(ix)
        self.seen = []

    def exact(self, ids, query):
        d = super().exact(ids, query)
        if len(ids):
            self.seen.append((np.array(ids, np.uint32), d.copy()))
        return d


def _supported(lib):
    fn = lib.bang_search_exact_supported
    fn.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    fn.restype = C.c_int
    return fn


@pytest.mark.parametrize("name", H.NAMES)
def test_input_runs_on_the_reference_and_reaches_its_ground(name):
    ix, q = H.get(name)
    eight_bit = ix.dtype != "float"
    for L in H.LS:
        for i in range(q.shape[0]):
            ref = _Recording(ix)
            ids, d, st = ref.search_one(q[i], 10, L, "exact")
            assert st[0] <= L + 49 and st[2] >= 1
            assert (ids != np.iinfo(np.uint64).max).all() and np.all(np.diff(d) >= 0)
            if not eight_bit:
                continue
            sid = np.concatenate([s for s, _ in ref.seen])
            chain = np.concatenate([c for _, c in ref.seen])
            sums = H.integer_sums(ix, sid, q[i])
            differs = chain.view(np.uint32) != sums.astype(np.float32).view(np.uint32)
            if name in H.FAR:
                assert (sums >= H.TWO24).all() and (chain >= np.float32(H.TWO24)).all()
                assert differs.any(), (name, L, i)                       # the chain rounds: the integer sum is not its value
            else:
                assert not differs.any(), (name, L, i)


@pytest.mark.parametrize("name", H.NAMES)
def test_inputs_lie_outside_the_old_ground_and_inside_the_new(name, libbang):
    ix, _ = H.get(name)
    libbang.bang_search_can_rerank.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32]
    assert libbang.bang_search_can_rerank(O.DTYPE_CODE[ix.dtype], ix.D, ix.entry_len, 0) == 0
    assert _supported(libbang)(O.DTYPE_CODE[ix.dtype], ix.D, ix.entry_len) == 1


def test_layout_predicate_refuses_what_the_kernels_do_not_evaluate(libbang):
    ok = _supported(libbang)
    u8, f32 = O.DTYPE_CODE["uint8"], O.DTYPE_CODE["float"]
    entry = lambda vec_bytes, R=32: vec_bytes + 4 + 4 * R                # noqa: E731
    assert ok(u8, 40, entry(40)) == 0                                    # 8-bit: D % 16 != 0
    assert ok(f32, 1028, entry(4 * 1028)) == 0                           # D > 1024
    assert ok(f32, 962, entry(4 * 962)) == 0                             # float: D % 4 != 0
    assert ok(u8, 784, entry(784) + 2) == 0                              # an entry stride not divisible by 4
    assert ok(f32, 960, entry(4 * 960) + 1) == 0
    assert ok(u8, 1040, entry(1040)) == 0
    for dt, D in ((u8, 16), (u8, 128), (u8, 784), (u8, 1024), (f32, 4), (f32, 256), (f32, 260), (f32, 1024)):   # old and new ground
        assert ok(dt, D, entry(D * (4 if dt == f32 else 1))) == 1, (dt, D)


def test_predicate_is_declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    assert re.search(r"^int\s+bang_search_exact_supported\s*\(\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;", src, flags=re.M)


def test_wide_instances_run_without_scratch(libbang, tmp_path):
    """One wide instance per vector type (u8 / i8 / f32), no scratch -- read from the code object's kernel descriptors (ELF notes)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    obj = os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "bang_search_exact_wide.o")
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    assert os.path.exists(obj), obj
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", obj, str(tmp_path / "unused.o")], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split(".name:")[1:]:
        m = re.match(r"_Z24search_exact_wide_kernelILi(\d)EEv9ExactArgs$", blk.split()[0])
        if m:
            found[int(m.group(1))] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)),
                                      int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1)))
    print("wide instances (scratch bytes, VGPRs):", found)
    assert sorted(found) == [0, 1, 2], found
    assert all(v[0] == 0 for v in found.values()), found
