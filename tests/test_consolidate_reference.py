"""The consolidation inputs reach their edges and the CPU reference keeps the graph's invariants (no GPU): what tests/test_gpu_consolidate.py
compares the engine against, byte for byte, is worth comparing against.

Run time of the reference on one CPU core, measured (Reference.exact, one ctypes call per id, is fast enough: no vectorised distance was needed):
"deep_ball4" 0.8 s, "cut_ball12" 0.5 s, "i8_ball24" 0.4 s, every other case 0.15 s or less."""
import numpy as np
import pytest

import consolidate_inputs as CI
import consolidate_reference as CR
import insert_inputs as I


@pytest.mark.parametrize("name", sorted(CI.CASES))
def test_invariants_of_the_consolidated_index(name):
    ix, x, alpha = CI.case(name)
    ix2, st, remaining = CI.reference(name)
    in_d, rem = CR.split(ix, x)
    assert np.array_equal(remaining, rem) and st["still_excluded"] == len(rem) and st["removed"] == int(in_d.sum())
    assert ix2.N == ix.N and ix2.medoid == ix.medoid and np.array_equal(ix2.codes, ix.codes)
    assert np.array_equal(ix2.vectors(), ix.vectors()), "vectors stay, those of removed nodes included"
    deg, adj = ix2.degrees(), ix2.adjacency()
    old_rows = CR.rows_of(ix)
    assert not deg[in_d].any() and not adj[in_d].any(), "removed rows are R + 1 zero words"
    affected = set(int(p) for p in st["affected"])
    assert st["rows"] == len(affected) > 0
    for p in range(ix.N):
        row = adj[p, :deg[p]]
        assert not in_d[row].any(), f"live row {p} lists a removed node"
        assert not adj[p, deg[p]:].any(), "unused slots are 0"
        if in_d[p]:
            continue
        if p in affected:
            assert p not in row and len(np.unique(row)) == len(row)
            pool = set(int(c) for c in old_rows[p]) | set(int(c) for v in old_rows[p][in_d[old_rows[p]]] for c in old_rows[int(v)])
            assert set(int(c) for c in row) <= pool
        else:
            assert np.array_equal(ix2.graph[p], ix.graph[p]), "an unaffected entry is unchanged byte for byte"


def test_the_i8_ball_reaches_duplicates_p_in_removed_rows_and_the_medoid_row():
    ix, x, _ = CI.case("i8_ball24")
    cl = CR.lists(ix, x)
    assert 300 <= len(cl) <= 450
    assert sum(len(np.unique(c.ids)) < len(c.ids) for c in cl.values()) >= 100, "lists with duplicates"
    assert sum(c.lists_p for c in cl.values()) >= 20, "a removed row that lists p"
    assert all(c.removed_lists_removed for c in cl.values()), "every removed row lists removed nodes"
    assert max(len(np.unique(c.ids)) for c in cl.values()) >= 150
    assert any(c.n_removed >= 2 for c in cl.values())
    assert int(ix.medoid) in cl and ix.medoid not in x, "the medoid's row is affected, the medoid is live"
    assert CI.reference("i8_ball24")[1]["dropped"] == 0


def test_the_medoid_inside_the_set_stays_a_routing_node():
    ix, x, _ = CI.case("i8_ball8_med")
    ix2, st, remaining = CI.reference("i8_ball8_med")
    med = int(ix.medoid)
    assert med in x and list(remaining) == [med] and st["removed"] == 7 and st["still_excluded"] == 1
    assert med in st["affected"], "the medoid's row is repaired like any other"
    assert ix2.degrees()[med] > 0 and not np.array_equal(ix2.graph[med], ix.graph[med])
    assert (ix2.adjacency()[ix2.degrees() > 0] == med).any(), "live rows may still list the medoid"


def test_the_cut_at_512_is_reached():
    ix, x, _ = CI.case("cut_ball12")
    cl = CR.lists(ix, x)
    over = [len(c.ids) - 512 for c in cl.values() if len(c.ids) > 512]
    assert len(over) >= 5 and len(cl) >= 200
    assert CI.reference("cut_ball12")[1]["dropped"] == sum(over)


def test_the_crafted_graph_has_an_affected_node_whose_list_ends_empty():
    ix, x = CI.sparse()
    cl = CR.lists(ix, x)
    assert len(cl[CI.SPARSE_EMPTY].ids) == 0 and cl[CI.SPARSE_EMPTY].lists_p and cl[CI.SPARSE_EMPTY].removed_lists_removed
    assert list(cl[CI.SPARSE_ONE].ids) == [30, 30, CI.SPARSE_EMPTY], "a list shorter than R, with a duplicate"
    ix2, st, _ = CI.reference("sparse")
    vb = ix.D
    assert not ix2.graph[CI.SPARSE_EMPTY, vb:].any(), "an empty list gives degree 0 and zero slots"
    row = ix2.graph[CI.SPARSE_ONE, vb:].view(np.uint32)
    assert row[0] in (1, 2) and set(int(c) for c in row[1: 1 + row[0]]) <= {30, CI.SPARSE_EMPTY} and not row[1 + row[0]:].any()
    assert CI.SPARSE_EMPTY in st["affected"]


@pytest.mark.parametrize("kind", sorted(I.LATTICES))
def test_a_strict_kill_rule_would_change_a_row_on_the_lattices(kind):
    name = "lattice_" + kind
    ix, x, alpha = CI.case(name)
    ix2, st, _ = CI.reference(name)
    wrong, _, _ = CR.consolidate(ix, x, alpha, strict=True)
    differ = [int(p) for p in st["affected"] if not np.array_equal(wrong.graph[p], ix2.graph[p])]
    assert differ, "'<' and '<=' give the same rows: the input does not pin the kill rule"


def test_every_layout_case_is_busy():
    for k in sorted(I.LAYOUTS):
        ix, x, _ = CI.case("layout_" + k)
        _, st, _ = CI.reference("layout_" + k)
        assert 150 <= st["rows"] <= 290 and st["removed"] in (29, 30), (k, st["rows"])


def test_the_scan_graph_is_what_its_docstring_says():
    for R in (5, 16, 64):
        graph, med, excluded, want, bad_node, bad_id = CI.scan_graph(R)
        rows = graph[:, 16:].view(np.uint32)
        gone = set(int(v) for v in excluded) - {med}
        got = []
        for p in range(CI.SCAN_N):
            if p in gone:
                continue
            ids = list(rows[p, 1: 1 + min(int(rows[p, 0]), R)])
            if bad_id in ids:
                ids = ids[:ids.index(bad_id)]
            assert all(i < CI.SCAN_N for i in ids)
            if gone & set(int(i) for i in ids):
                got.append(p)
        assert got == list(want)
        assert rows[0, 0] == 0 and rows[1, 0] == R and rows[5, 0] > R and rows[2, 1] in gone and rows[4, R] in gone
