"""The insert inputs reach their edges and the CPU reference keeps the graph's invariants (no GPU): what tests/test_gpu_insert.py compares the
engine against, bit for bit, is worth comparing against."""
import numpy as np
import pytest

import insert_inputs as I
import insert_reference as IR
from exact_reference import Reference


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_invariants_of_the_grown_index(name):
    ix, v, L, alpha = I.case(name)
    ix2, st = I.reference(name)
    n, N, R = len(v), ix.N, ix.R
    assert ix2.N == N + n and ix2.graph.shape == (N + n, ix.entry_len) and ix2.codes.shape == (N + n, ix.m)
    assert st["inserted"] == n
    deg, adj = ix2.degrees(), ix2.adjacency()
    assert deg.max() <= R
    for x in range(N + n):
        row = adj[x, :deg[x]]
        assert x not in row, f"self-loop at {x}"
        assert len(np.unique(row)) == len(row), f"node {x} lists an id twice"
        assert row.max(initial=0) < N + n
        assert not adj[x, deg[x]:].any(), "unused slots are 0"
    # old vectors and codes untouched, new vectors those of the batch, medoid where it was
    assert np.array_equal(ix2.vectors()[:N], ix.vectors()) and np.array_equal(ix2.vectors()[N:], v)
    assert np.array_equal(ix2.codes[:N], ix.codes)
    assert ix2.medoid == ix.medoid
    # rows of new nodes list old nodes only; an old row changed only by gaining new ids or by a prune of old row ++ new ids
    assert adj[N:][np.arange(R)[None, :] < deg[N:, None]].max() < N
    old_adj, old_deg = ix.adjacency(), ix.degrees()
    for x in range(N):
        gained = set(adj[x, :deg[x]]) - set(old_adj[x, :old_deg[x]])
        assert all(g >= N for g in gained)


def test_new_rows_end_short_of_R_at_alpha_1_2_and_stop_full_at_alpha_8():
    for name, (iname, n, L, alpha, _) in I.CASES.items():
        ix, _ = I.get(iname)
        ix2, _ = I.reference(name)
        new = ix2.degrees()[ix.N:]
        if alpha == 1.2:
            assert new.min() >= 1 and new.max() < ix.R, name
        else:
            assert alpha == 8.0 and L > ix.R and (new == ix.R).all(), name


def test_both_back_edge_paths_a_changed_medoid_row_and_a_busy_target():
    appended = pruned = 0
    for name in I.CASES:
        _, st = I.reference(name)
        assert st["appended"] > 0 and st["pruned"] > 0, (name, st)
        assert st["dropped"] == 0                                         # (R + n <= 512 here: insert_inputs.DUP is the batch that meets the cap)
        appended += st["appended"]
        pruned += st["pruned"]
    assert appended >= 200 and pruned >= 200
    assert any(I.reference(name)[1]["medoid_row_changed"] for name in I.CASES)
    assert any(I.reference(name)[1]["max_incoming"] >= 3 for name in I.CASES)
    # the medoid's row really differs where the reference says so
    ix, _, _, _ = I.case("u8_a12")
    ix2, st = I.reference("u8_a12")
    assert st["medoid_row_changed"] and not np.array_equal(ix2.graph[ix.medoid], ix.graph[ix.medoid])


@pytest.mark.parametrize("name", ["i8_a12", "deep_a12"])
def test_a_candidate_at_distance_zero(name):
    """the exact duplicates (and the medoid's copy) meet their originals at distance 0: alpha2 * e <= d_t with both sides 0"""
    ix, v, L, _ = I.case(name)
    ref = Reference(ix)
    zero = 0
    for i in range(len(v) - 5, len(v)):
        ids, d = IR.candidates(ref, v[i], L)
        zero += int((d == 0).any())
    assert zero >= 1


def test_prune_rules_on_a_hand_made_list():
    ix, _ = I.get("i8")
    ref = Reference(ix)
    ids = np.array([5, 9, 5, 700, 9], np.uint32)                          # ids twice: the copy dies at e = 0
    d = ref.exact(ids, IR.vector_of(ref, 3))
    order = np.argsort(d, kind="stable")
    out = IR.prune(ref, 9, ids[order], d[order], ix.R, IR.alpha2_of(1.0))
    assert 9 not in out and len(set(out)) == len(out) and len(out) >= 1
    assert list(IR.prune(ref, 1 << 30, ids[order], d[order], 1, IR.alpha2_of(1.0))) == [ids[order][0]]     # stops at R
    assert len(IR.prune(ref, 0, np.zeros(0, np.uint32), np.zeros(0, np.float32), ix.R, IR.alpha2_of(1.2))) == 0
    assert IR.alpha2_of(1.2) == np.float32(np.float32(1.2) * np.float32(1.2))


def test_codes_are_the_lowest_argmin_of_the_lut():
    ix, v, _, _ = I.case("u8_a12")
    ix2, _ = I.reference("u8_a12")
    ref = Reference(ix)
    for i in (0, len(v) - 1):
        lut = ref.orc.lut_build(v[i])
        code = ix2.codes[ix.N + i]
        for c in range(ix.m):
            assert lut[c, code[c]] == lut[c].min() and not (lut[c, :code[c]] == lut[c].min()).any()
    assert ix2.codes.dtype == np.uint8


def test_a_target_with_more_candidates_than_the_cap_loses_the_tail_of_its_incoming_ids():
    ix, v, L, alpha, ix2, st = I.dup_reference()
    node, R = I.DUP[4], ix.R
    deg, adj = ix2.degrees(), ix2.adjacency()
    assert (adj[ix.N:, 0] == node).all(), "every copy picks its original first (distance 0)"
    assert (adj[ix.N:] == adj[ix.N]).all()                                # equal vectors, equal rows: every target of the row has 500 incoming ids
    targets = adj[ix.N, :deg[ix.N]]
    over = ix.degrees()[targets].astype(np.int64) + len(v) - IR.PRUNE_MAX
    assert st["max_incoming"] == len(v) and st["dropped"] == over[over > 0].sum() > 0 and over[0] > 0
    row = adj[node, :deg[node]]
    assert deg[node] <= R and len(np.unique(row)) == len(row) and (row >= ix.N).sum() >= 1
    assert row[row >= ix.N].max() < ix.N + IR.PRUNE_MAX - ix.degrees()[node], "an id of the dropped tail made it into the row"


def test_the_reference_applied_twice_sees_the_first_batch():
    ix1, _ = I.reference("i8_a12")
    v2, ix2, st = I.second_reference()
    assert ix2.N == ix1.N + len(v2) and st["inserted"] == len(v2)
    new_rows = ix2.adjacency()[ix1.N:]
    base_n = I.get("i8")[0].N
    assert (new_rows >= base_n).any(), "no point of the second batch lists a point of the first: the second call must see the first"
