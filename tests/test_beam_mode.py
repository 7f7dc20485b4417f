"""The beam form of the exact-distance walk (options "distance" = 1, "beam" = W) -- what can be checked without a GPU: the CPU reference
(tests/beam_reference.py) against answers derived by hand, the edge inputs of tests/beam_inputs.py against the edges they are named for,
what a beam does to the walk on a fixture, the option, and the code objects of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_inputs as BI
from beam_reference import Reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = int(np.iinfo(np.uint64).max)


def _one(ix, q, k, L, W):
    trace = []
    ids, d, st, cand = Reference(ix).search_one(q[0], k, L, W, trace)
    return ids.tolist(), d, tuple(int(x) for x in st), cand.tolist(), trace


# ------------------------------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_shared_child_known_answer(dtype, D):
    """W = 2, L = 8.  it 1: T = [0, 1, 2] -> worklist 1, 2, 0 (0 visited); parents 1, 2.  it 2: rows [3, 4] and [3, 5]: all four ids pass the
    filter state at entry, the 3 of row 1 is dropped: S_0 = [3, 4], S_1 = [5] -> worklist 3, 5, 4, 1, 2, 0; parents 3, 5.  it 3: two empty rows;
    parent 4.  it 4: an empty row, nothing unvisited: the end."""
    ix, q = BI.shared_child(dtype, D)
    ids, d, st, cand, trace = _one(ix, q, 8, 8, 2)
    assert cand == [0, 1, 2, 3, 5, 4]
    assert ids == [3, 5, 4, 1, 2, 0, PAD, PAD]
    assert d[:6].tolist() == [float(D * v * v) for v in (10, 12, 15, 20, 30, 100)]
    assert st == (4, 6, 6, 7)                                   # iterations, candidates, dist_evals (3 + 3), fetched (3 + 4 + 0 + 0)
    assert trace[1]["dropped"] == 1 and trace[1]["kept"] == [2, 1] and ids.count(3) == 1


@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_row_tie_known_answer(dtype, D):
    """W = 2, L = 8.  it 2: rows [3] and [4], equal distances: row 0's 3 is merged first, row 1's 4 then enters IN FRONT of it (new before
    equal old): worklist 4, 3, 1, 2, 0; parents 4, 3 in that order.  it 3: two empty rows, nothing unvisited."""
    ix, q = BI.row_tie(dtype, D)
    ids, d, st, cand, trace = _one(ix, q, 8, 8, 2)
    assert cand == [0, 1, 2, 4, 3]
    assert ids == [4, 3, 1, 2, 0, PAD, PAD, PAD]
    assert d[0] == d[1] == float(D * 100)
    assert st == (3, 5, 5, 5)                                   # dist_evals 3 + 2, fetched 3 + 2 + 0
    # at L = 3 the tie decides who stays: 4, 3 and then node 1
    assert _one(ix, q, 3, 3, 2)[0] == [4, 3, 1]


# ------------------------------------------------------------------------------------------------------------------------ the edges are reached
@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_row_dup_both_copies_stay_and_the_second_row_is_dropped(dtype, D):
    ix, q = BI.row_dup(dtype, D)
    ids, _, st, cand, trace = _one(ix, q, 8, 8, 2)
    assert trace[1]["kept"] == [3] and ids[:6] == [4, 5, 2, 2, 3, 1]     # duplicates inside one row stay
    assert trace[1]["parents"] == [2, 2]
    assert trace[2]["rows"] == 2 and trace[2]["kept"] == [2, 0] and trace[2]["dropped"] == 2
    assert ids.count(4) == 1 and ids.count(5) == 1


@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_ladder_fills_the_candidate_log_with_half_a_beam(dtype, D):
    ix, q = BI.ladder(dtype, D)
    L = BI.LADDER_L
    _, _, st, cand, trace = _one(ix, q, L, L, 2)
    assert all(t["P"] == 2 for t in trace[:29])
    last = trace[29]
    assert last["room"] == 1 and last["unvisited"] == 2 and last["P"] == 1       # P < min(W, unvisited)
    assert st[1] == L + 50 and trace[-1]["P"] == 0 and trace[-1]["unvisited"] >= 1
    assert st[0] == 31 < L + 49                                                   # (the log ends the query, not the iteration cap)


@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_fan4_keeps_256_survivors_in_one_iteration(dtype, D):
    ix, q = BI.fan4(dtype, D)
    _, d, st, _, trace = _one(ix, q, 37, 37, 4)
    assert trace[1]["rows"] == 4 and trace[1]["kept"] == [64, 64, 64, 64] and trace[1]["dropped"] == 0
    assert (np.diff(d) == 0).any()                                                # ties among the first results
    assert _one(ix, q, 37, 37, 2)[4][1]["kept"] == [64, 64]


@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_chain_runs_to_the_cap_with_a_full_log(dtype, D):
    ix, q = BI.build("chain", dtype, D)[:2]
    for W in (2, 4):
        for L in (10, 37):
            _, _, st, cand, trace = _one(ix, q, L, L, W)
            assert st[0] == L + 49 and st[1] == L + 50 and cand == list(range(L + 50))
            assert all(t["P"] == 1 for t in trace)


@pytest.mark.parametrize("dtype,D", BI.LAYOUTS)
def test_seed65_and_short_worklist(dtype, D):
    ix, q = BI.build("seed65_best", dtype, D)[:2]
    _, _, st, cand, trace = _one(ix, q, 4, 4, 2)
    assert trace[0]["kept"] == [65] and cand[1:3] == [64, 3]                      # the 65th id first, then the first of the two equal minima
    ix, q = BI.build("short_worklist", dtype, D)[:2]
    ids, _, st, _, _ = _one(ix, q, 10, 16, 2)
    assert ids == [1, 2, 0] + [PAD] * 7


def test_every_input_is_built_in_every_vector_type():
    names = {c[0] for c in BI.cases()}
    assert names == set(BI.INPUTS)
    for name in BI.INPUTS:
        want = 2 if name == "extreme" else 3
        assert sum(1 for c in BI.cases() if c[0] == name) == want


# ------------------------------------------------------------------------------------------------------------------------ a fixture
def test_a_beam_of_four_more_than_halves_the_iterations(small_u8):
    ix, q, _, _ = small_u8
    ref = Reference(ix)
    L, k = 37, 10
    its = {}
    for W in (1, 2, 3, 4):
        ids, d, st, log = ref.search(q, k, L, W)
        its[W] = float(st[:, 0].mean())
        for i in range(q.shape[0]):
            row = ids[i].tolist()
            assert len(set(row)) == k, (W, i, row)                                # no id repeats among a query's first k results
            assert np.all(np.diff(d[:, i]) >= 0)
            assert log[i, 0] == ix.medoid and len(set(log[i, :st[i, 1]].tolist())) == st[i, 1]
    print("iterations per query:", its)
    assert its[4] < 0.5 * its[1], its
    assert its[4] < its[2] < its[1]


def test_beam_one_expands_one_node_per_iteration(small_i8):
    """W = 1 is the post-merge-parent walk: every iteration but a query's last logs exactly one parent, and the log never exceeds L + 50."""
    ix, q, _, _ = small_i8
    L = 10
    _, _, st, log = Reference(ix).search(q[:8], 10, L, 1)
    for i in range(8):
        it, cand = int(st[i, 0]), int(st[i, 1])
        assert cand in (it, it + 1) and cand <= L + 50, (it, cand)          # it parents + the medoid, less one where the walk ran dry
        assert len(set(log[i, :cand].tolist())) == cand


# ------------------------------------------------------------------------------------------------------------------------ option, ABI, code objects
def test_beam_option_is_in_the_table_and_range_checked(libbang):
    lib = libbang
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    text = buf.value.decode()
    assert re.search(r"^  beam\s+BANG_BEAM\s+\[1, 4\]\s+bang_alloc\s", text, flags=re.M)
    entry = text[text.index("\n  beam"):]
    entry = entry[:entry.index("\n  semantics")]
    for word in ("distance = 1", "semantics = 1", "vectors_fp16", "wide"):
        assert word in entry, word
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == 0
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    try:
        assert lib.bang_set_option(h, b"beam", 1) == 0
        assert lib.bang_set_option(h, b"beam", 4) == 0
        assert lib.bang_set_option(h, b"beam", 0) != 0
        assert lib.bang_set_option(h, b"beam", 5) != 0
    finally:
        lib.bang_destroy.argtypes = [C.c_void_p]
        lib.bang_destroy(h)


@pytest.mark.parametrize("obj,kernel", [("bang_search_beam.o", "search_exact_beam_kernel"), ("bang_search_beam_pull.o", "search_exact_beam_pull_kernel")])
def test_beam_instances_run_without_scratch_in_128_registers(libbang, tmp_path, obj, kernel):
    """One instance per vector type in each of the two builds: no scratch, at most 128 VGPRs (16 waves per CU) -- from the kernel descriptors."""
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
        m = re.match(r"_Z\d+" + kernel + r"ILi(\d)EEv8BeamArgs$", blk.split()[0])
        if m:
            found[int(m.group(1))] = (int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1)),
                                      int(re.search(r"\.vgpr_count:\s*(\d+)", blk).group(1)))
    assert sorted(found) == [0, 1, 2], found
    assert all(s == 0 and v <= 128 for s, v in found.values()), found
