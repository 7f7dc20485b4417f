"""BANG_Inmemory search semantics (option "semantics" = 1) -- what can be checked without a GPU: the option, the exported kernel, its code
objects, the CPU reference composition the GPU tests compare against (tests/inmemory_reference.py) and hand-made cases whose answers under
the two walks are known."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from inmemory_reference import Reference, chain_index, medoid_tie_index, medoid_tie_variant, not_full_index, tie_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _options(lib):
    lib.bang_describe_options.argtypes = [C.c_char_p, C.c_size_t]
    need = lib.bang_describe_options(None, 0)
    buf = C.create_string_buffer(need)
    lib.bang_describe_options(buf, need)
    return buf.value.decode()


def test_semantics_option_is_in_the_table_and_range_checked(libbang):
    lib = libbang
    assert re.search(r"^  semantics\s+BANG_SEMANTICS\s+\[0, 1\]\s+bang_alloc\s", _options(lib), flags=re.M)
    h = C.c_void_p()
    assert lib.bang_create(0, C.byref(h)) == 0
    lib.bang_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
    try:
        assert lib.bang_set_option(h, b"semantics", 0) == 0
        assert lib.bang_set_option(h, b"semantics", 1) == 0
        assert lib.bang_set_option(h, b"semantics", 2) != 0
        assert lib.bang_set_option(h, b"semantics", -1) != 0
    finally:
        lib.bang_destroy.argtypes = [C.c_void_p]
        lib.bang_destroy(h)


def test_environment_words_are_documented_and_parsed_through_the_table(libbang):
    """BANG_SEMANTICS takes the words base | inmemory (or 0 / 1); the parse sits in the option table's environment pass (bang_options.cpp),
    the only place the engine reads its environment.  (That the words take effect is checked on the GPU: tests/test_gpu_inmemory.py.)"""
    line = [l for l in _options(libbang).splitlines() if l.strip().startswith("semantics ")]
    assert len(line) == 1 and "(environment: base | inmemory)" in line[0], line
    src = open(os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc", "bang_options.cpp")).read()
    body = src[src.index("void apply_env_defaults"):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"&bang_engine::semantics.*\n\s*x = strcmp\(v, \"inmemory\"\) == 0 \? 1 : 0;", body), body


def test_python_constants():
    import bang_amd
    assert (bang_amd.SEMANTICS_BASE, bang_amd.SEMANTICS_INMEMORY) == (0, 1)


def test_inmem_kernel_is_declared_and_exported(libbang):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bang_c.h")).read(), flags=re.S)
    for name in ("bang_k_search_inmem", "bang_search_inmem_geometry"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert hasattr(libbang, name), name
    assert re.search(r"int\s+bang_k_search_inmem\s*\(\s*const\s+bang_search_params\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"#define\s+BANG_INMEM_EXTRA_ITERS\s+120\b", src)


def test_inmem_kernel_instances_run_without_scratch(libbang, tmp_path):
    """Self-paced instances only (HOST = SPEC = false), each in exactly one of the two translation units, none with scratch --
    read from the code objects' kernel descriptors (ELF notes)."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    objs = [os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", n) for n in ("bang_search_inmem.o", "bang_search_inmem_b.o")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("llvm binutils are not here")
    for o in objs:
        assert os.path.exists(o), o
    found = []
    for tag, obj in enumerate(objs):
        fat, co = str(tmp_path / f"fat{tag}.bin"), str(tmp_path / f"dev{tag}.co")
        subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", obj, str(tmp_path / "unused.o")], check=True)
        subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
        notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
        part = {}
        for blk in notes.split(".name:")[1:]:
            name = blk.split()[0]
            assert "search_kernel" not in name or "search_inmem_kernel" in name, name     # the base instances stay in bang_search(_b).o
            m = re.match(r"_Z19search_inmem_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELb([01])ELb([01])EEv10SearchArgs$", name)
            if m:
                key = tuple(int(x) for x in m.groups())                      # (PSZ, NDW, ALIGNED, NHI, HOST, SPEC)
                part[key] = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
        found.append(part)
    assert found[0] and found[1] and not (set(found[0]) & set(found[1]))
    allk = {**found[0], **found[1]}
    assert all(k[4] == 0 and k[5] == 0 for k in allk), sorted(allk)
    assert all(v == 0 for v in allk.values()), allk
    for key in [(2, 18, 1, 58, 0, 0), (2, 19, 1, 22, 0, 0), (4, 8, 1, 0, 0, 0), (4, 8, 0, 0, 0, 0)]:     # the BASELINE layouts
        assert key in allk, key


FIXTURES = ("small_u8", "small_f32", "small_i8", "small_deep")


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("L", [10, 37, 152])
def test_base_composition_equals_the_oracle(name, L, request):
    """The composition in `base` mode IS the oracle's search, bit for bit: ids, distance bits and per-query statistics."""
    from oracle import oracle as O
    ix, q, _, _ = request.getfixturevalue(name)
    q = q[:16]
    ids_o, d_o, st_o = O.Oracle(ix).search(q, 10, L, with_stats=True)
    ids, d, st = Reference(ix).search(q, 10, L, "base")
    assert np.array_equal(ids, ids_o)
    assert np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
    assert np.array_equal(st, st_o)


def _known(ix, q, k, L, mode, ids, stats):
    from oracle import oracle as O
    got_ids, got_d, st = Reference(ix).search(q, k, L, mode)
    assert got_ids[0].tolist() == ids, (mode, got_ids[0].tolist())
    assert st[0].tolist() == stats, (mode, st[0].tolist())
    lv = ix.graph[:, 0].astype(np.float32)                               # (toy_index: exact distance = 128 level^2)
    assert np.array_equal(got_d[:, 0], (128.0 * lv[got_ids[0].astype(np.int64)] ** 2).astype(np.float32))
    if mode == "base":
        ids_o, _, st_o = O.Oracle(ix).search(q, k, L, with_stats=True)
        assert ids_o[0].tolist() == ids and st_o[0].tolist() == stats


def test_tie_between_best_survivor_and_worklist_head():
    # iteration 2: survivor 3 ties with the unvisited entry 2.  BANG_Base expands 2 (strict '<'), reaches 4, then 3 and 5: six
    # candidates.  The merge puts 3 first; at L = 3 node 2 is evicted by 5 and never expanded: candidates 0, 1, 3, 5.
    ix, q = tie_index()
    _known(ix, q, 3, 3, "base", [4, 5, 1], [6, 6, 6, 6])
    _known(ix, q, 3, 3, "inmemory", [5, 1, 3], [4, 4, 5, 5])


def test_not_full_worklist_without_unvisited_entries():
    # iteration 2: worklist {1, 0} all visited, survivor 2 behind the tail.  BANG_Base merges it and expands it one iteration later
    # (an iteration without a parent); the merge-first rule expands it at once: 5 against 4 iterations, the same candidates.
    ix, q = not_full_index()
    _known(ix, q, 3, 10, "base", [3, 1, 0], [5, 4, 4, 4])
    _known(ix, q, 3, 10, "inmemory", [3, 1, 0], [4, 4, 4, 4])


def test_medoid_ties_the_best_neighbour():
    # iteration 1: medoid 0 and node 1 share level 10; sorted, the medoid (input position 0) comes first.  The parent is node 1 at slot 1,
    # marked there: it is expanded once (candidates 0, 1, 3, 2, 4).  Marking slot 0 instead would leave node 1 unvisited and expand it twice.
    ix, q = medoid_tie_index()
    _known(ix, q, 5, 10, "base", [3, 4, 0, 1, 2], [5, 5, 5, 5])
    _known(ix, q, 5, 10, "inmemory", [3, 4, 0, 1, 2], [5, 5, 5, 5])


def test_medoid_tie_variant_of_small_u8_expands_no_node_twice(small_u8):
    """The fixture the GPU parity test runs with the medoid tying its best neighbour: the reference logs no candidate twice and no
    query returns an id twice."""
    ix, q, _, _ = small_u8
    from oracle import oracle as O
    ix2, q2, j = medoid_tie_variant(ix, q[:4])
    ref = Reference(ix2)
    T = np.concatenate([[ix2.medoid], ref.adjacency(ix2.medoid)]).astype(np.uint32)
    S, d = O.sort_pairs(T, ref.orc.pqdist(ref.orc.lut_build(q2[0]), T))
    assert S[:2].tolist() == [ix2.medoid, j] and d[0] == d[1]           # iteration 1: the medoid sorts first, tied with the parent
    for L in (10, 37):
        ids, _, st = ref.search(q2, 10, L, "inmemory")
        for i in range(q2.shape[0]):
            assert len(set(ids[i].tolist())) == 10
            assert st[i][1] == st[i][0] + 1 or st[i][1] == st[i][0]      # one candidate per iteration (+ the medoid), none repeated


@pytest.mark.parametrize("L", [10, 37])
def test_chain_runs_to_the_cap(L):
    # the distance falls along the chain: every iteration expands the next node until the cap, L + 49 (base) / L + 119 (inmemory);
    # the parent picked at the cap is logged (candidates = iterations + 1) but not expanded (dist_evals = fetched = candidates)
    ix, q = chain_index()
    for mode, cap in (("base", L + 49), ("inmemory", L + 119)):
        _known(ix, q, 10, L, mode, list(range(cap, cap - 10, -1)), [cap, cap + 1, cap + 1, cap + 1])


@pytest.mark.parametrize("name", FIXTURES)
def test_inmemory_reference_is_self_consistent(name, request):
    from oracle import oracle as O
    ix, q, gt_i, gt_d = request.getfixturevalue(name)
    ref = Reference(ix)
    L = 37
    ids, d, st = ref.search(q, 10, L, "inmemory")
    for i in range(q.shape[0]):
        assert np.all(np.diff(d[:, i]) >= 0)
        assert 1 <= st[i][0] <= L + 119 and st[i][1] <= st[i][0] + 1
    rec = O.recall(gt_i, gt_d, ids, 10)
    ids_b, _, _ = ref.search(q, 10, L, "base")
    print(f"{name}: 10-recall@10 at L = {L}: inmemory {rec:.1f} %, base {O.recall(gt_i, gt_d, ids_b, 10):.1f} %")
    assert rec > 0.0
