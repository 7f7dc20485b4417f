"""tests/fp16_inputs.py on the CPU: the helper is not vacuous.  On every float input tests/test_gpu_vectors_fp16.py compares the engine with,
the reference on the index with its vectors rounded to fp16 differs from the reference on the original index in at least one distance bit
pattern -- an engine that ignored option vectors_fp16 could not pass the GPU comparison -- and the inputs reach the edges they are named for."""
import numpy as np
import pytest

import edge_inputs as E
import fp16_inputs as H


def test_rounded_changes_the_vectors_and_nothing_else(small_deep):
    ix = small_deep[0]
    r = H.rounded(ix)
    assert np.array_equal(r.vectors(), ix.vectors().astype(np.float16).astype(np.float32)) and not np.array_equal(r.vectors(), ix.vectors())
    assert np.array_equal(r.adjacency(), ix.adjacency()) and np.array_equal(r.degrees(), ix.degrees())
    assert r.codes is ix.codes and r.pivots is ix.pivots and r.graph.shape == ix.graph.shape
    assert np.array_equal(H.rounded(r).graph, r.graph)                                   # idempotent: fp16 -> fp32 is exact
    assert [H.row_bytes(D) for D in (1, 7, 8, 96, 260)] == [4, 16, 16, 192, 520] and H.table_bytes(10, 7) == 416


@pytest.mark.parametrize("name", ["small_f32", "small_deep", "synth7", "synth33", "synth100", "synth260"])
def test_pq_walk_inputs_are_not_vacuous(name, request):
    ix, q = H.synth_index(int(name[5:])) if name.startswith("synth") else request.getfixturevalue(name)[:2]
    assert ix.dtype == "float" and ix.N <= 3000 and q.shape[0] <= 64
    want, orig = H.pq_reference((name, "r"), H.rounded(ix), q, 10, 37), H.pq_reference((name, "o"), ix, q, 10, 37)
    assert H.distance_bits_differ(want, orig)
    assert np.array_equal(want[2], orig[2])                   # (the walk runs on PQ distances: rounding reaches the re-rank alone)


def test_mips_input_is_not_vacuous(small_f32):
    ix, q = small_f32[:2]
    q1 = np.ascontiguousarray(q[:, :-1])
    assert H.distance_bits_differ(H.pq_reference(("small_f32", "r"), H.rounded(ix), q1, 10, 37, mips=True),
                                  H.pq_reference(("small_f32", "o"), ix, q1, 10, 37, mips=True))


def test_rounding_ties_exist_only_in_the_rounded_index(small_f32):
    ix, q = H.rounding_ties(*small_f32[:2])
    want, orig = H.pq_reference(("ties", "r"), H.rounded(ix), q, 10, 37), H.pq_reference(("ties", "o"), ix, q, 10, 37)
    assert H.distance_bits_differ(want, orig)
    assert E.ties_in_top(want[1], 10).any()
    # a pair (2j, 2j + 1) is one vector after rounding: where both are among a query's results they tie exactly, and only there
    ids, d = want[0], want[1].T
    hits = 0
    for qi in range(ids.shape[0]):
        pos = {int(x): r for r, x in enumerate(ids[qi])}
        for x, r in pos.items():
            if x % 2 == 0 and x + 1 in pos:
                assert d[qi, r] == d[qi, pos[x + 1]]
                hits += 1
    assert hits > 0


@pytest.mark.parametrize("name", ["small_deep", "synth256"])
def test_exact_mode_inputs_are_not_vacuous(name, request):
    ix, q = H.synth_index(256) if name == "synth256" else request.getfixturevalue(name)[:2]
    assert ix.D % 8 == 0 and ix.D <= 256
    assert H.distance_bits_differ(H.exact_reference((name, "r"), H.rounded(ix), q, 10, 37), H.exact_reference((name, "o"), ix, q, 10, 37))


@pytest.mark.parametrize("variant", E.SEED65_VARIANTS)
def test_off_grid_seed65_rounds_back_to_the_toy(variant):
    toy, q = E.seed65("float", variant, 128)
    ix = H.off_grid(toy)
    want = H.exact_reference(("seed65", variant, "r"), H.rounded(ix), q, 4, 10)
    assert H.distance_bits_differ(want, H.exact_reference(("seed65", variant, "o"), ix, q, 4, 10))
    ref_toy = H.exact_reference(("seed65", variant, "toy"), toy, q, 4, 10)
    assert all(np.array_equal(a, b) for a, b in zip(want, ref_toy))
    assert int(ix.degrees()[0]) == 64


def test_off_grid_chain_runs_to_the_cap():
    toy, q = E.chain("float", 128)
    ix = H.off_grid(toy)
    want = H.exact_reference(("chain", "r"), H.rounded(ix), q, 10, 10)
    assert want[2][0].tolist() == [59, 60, 60, 60]
    assert H.distance_bits_differ(want, H.exact_reference(("chain", "o"), ix, q, 10, 10))
