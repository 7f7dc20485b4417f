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


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the seam, layout, tie and search-form tests reach the edges they are named for
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(I.SEAMS))
def test_seam_cases_cross_their_seams_with_differing_data(name):
    ix, v, L, alpha, ix2, st = I.seam_case(name)
    sc, tc, ec = I.SEAMS[name]
    n = len(v)
    assert n > sc and n > ec, "no search / encode seam inside the batch"
    targets, pruned = st["targets"], st["target_pruned"]
    assert len(targets) > tc, "no target seam"
    assert (np.diff(targets.astype(np.int64)) > 0).all() and pruned.sum() == st["pruned"] and (~pruned).sum() == st["appended"]
    if tc == 1:                                                           # every target is a launch of its own: both paths, in launches behind the first
        assert pruned[1:].any() and not pruned[1:].all()
    else:
        for side in (pruned[:tc], pruned[tc:]):                           # both paths on both sides of the first target seam
            assert side.any() and not side.all(), name
    # behind EVERY seam the data differ from the same slots of the first chunk: a launch that took the first chunk's vectors or rows again would
    # show.  DUP_MIXED: chunks of copies of one vector cannot differ from each other; its chunks that hold distinct vectors are the ones asserted
    rows = ix2.graph[ix.N:, ix.D * (4 if ix.dtype == "float" else 1):]
    codes = ix2.codes[ix.N:]
    n_dup = n - I.DUP_MIXED_TAIL if name == "DUP_MIXED" else 0
    for what, table, chunk in (("rows", rows, sc), ("codes", codes, ec)):
        checked = 0
        for c0 in range(chunk, n, chunk):
            c1 = min(c0 + chunk, n)
            if c1 <= n_dup:
                continue
            assert any(not np.array_equal(table[x], table[x - c0]) for x in range(c0, c1)), (what, "chunk at", c0, "equals the first chunk")
            checked += 1
        assert checked >= 1 and (checked == (n - 1) // chunk or name == "DUP_MIXED"), (what, checked)
    if name == "DUP_MIXED":
        assert st["dropped"] > 0
        last = codes[(n - 1) // ec * ec:]
        assert len(np.unique(last, axis=0)) >= 2, "the last encode chunk holds one code row only"
        q_last = (n - 1) // sc * sc
        assert len(np.unique(rows[q_last:], axis=0)) >= 2 and len(np.unique(v[q_last:], axis=0)) >= 2


@pytest.mark.parametrize("name", sorted(I.LAYOUTS))
def test_layout_indexes_are_what_they_say(name):
    from bang_amd.binding import NP_DTYPE
    D, dtype, _ = I.LAYOUTS[name]
    ix = I.layout(name)
    assert (ix.N, ix.D, ix.R, ix.dtype) == (I.LAYOUT_N, D, I.LAYOUT_R, dtype)
    v = ix.vectors()
    assert v.dtype == NP_DTYPE[dtype] and len(np.unique(v, axis=0)) > ix.N // 2, "the vectors hardly differ: distances would not tell lanes apart"
    assert (v[:, -1] != v[0, -1]).any() and (v[:, 0] != v[0, 0]).any(), "the first or the last dimension is constant"
    assert (ix.degrees() == ix.R).sum() >= 2, "no two full rows: the back-edge test takes one to append to (cut short) and one that overflows"


def _rows(ref, lists, owns, R, alpha, **kw):
    return [tuple(IR.prune(ref, own, a, b, R, IR.alpha2_of(alpha), **kw)) for (a, b), own in zip(lists, owns)]


@pytest.mark.parametrize("iname", ["i8", "u8"])
def test_lattice_lists_pin_the_kill_rule_at_equality_and_at_float32_rounding(iname):
    # alpha = 1 on {0, 1, 2}^6: '<=' and '<' part ways on at least a third of the lists, and a kill happens at alpha2 * e == d_t exactly
    ix = I.lattice(iname, "tern6")
    ref = Reference(ix)
    assert len(np.unique(ix.vectors(), axis=0)) == I.LATTICE_N and ix.vectors()[:, 6:].max() == 0
    lists, owns = I.lattice_lists(iname, "tern6")
    assert sorted({len(a) for a, _ in lists}) == list(I.LATTICE_LENGTHS)
    ties = []
    le = [tuple(IR.prune(ref, own, a, b, ix.R, IR.alpha2_of(1.0), ties=ties)) for (a, b), own in zip(lists, owns)]
    lt = _rows(ref, lists, owns, ix.R, 1.0, strict=True)
    differ = sum(x != y for x, y in zip(le, lt))
    assert 3 * differ >= len(lists), differ
    assert sum(ties) >= 1
    # alpha = 1.2: fl32(1.44f * e) decides at least one comparison that the unrounded product decides the other way.  1.44f * e meets an integer
    # d_t that way at e = 25 (36), 50 (72), 100, 125 only -- {0, 1, 2}^6 ends at e = 24, so this is asserted on the lattice that reaches them
    a2 = IR.alpha2_of(1.2)
    assert np.float32(a2 * np.float32(25)) == 36 and float(a2) * 25 > 36 and np.float32(a2 * np.float32(50)) == 72 and float(a2) * 50 > 72
    ix = I.lattice(iname, "plane7")
    ref = Reference(ix)
    assert len(np.unique(ix.vectors(), axis=0)) == I.LATTICE_N
    lists, owns = I.lattice_lists(iname, "plane7")
    f32 = _rows(ref, lists, owns, ix.R, 1.2)
    f64 = _rows(ref, lists, owns, ix.R, 1.2, wide=True)
    assert any(x != y for x, y in zip(f32, f64)), "no comparison is decided by the rounding of alpha2 * e"


@pytest.mark.parametrize("name", sorted(I.PQ_LAYOUTS))
def test_pq_layout_ties_are_row_minima(name):
    ix, v = I.pq_layout(name)
    assert (ix.m, ix.D) == I.PQ_LAYOUTS[name] and v.shape == (9, ix.D)
    ref = Reference(ix)
    luts = np.stack([ref.orc.lut_build(x) for x in v])                    # [9][m][256]
    codes = np.stack([IR.encode(ref, x) for x in v])
    for lo, hi in I.PQ_TIES:
        assert lo < hi and np.array_equal(ix.pivots[lo], ix.pivots[hi])
        both = (luts[:, :, lo] == luts.min(axis=2)) & (luts[:, :, hi] == luts.min(axis=2))
        assert both.any(), (lo, hi, "the tie is nowhere the row minimum")
        assert (codes[both] == lo).all() and not (codes == hi).any()
    assert (I.PQ_TIES[0][1] - I.PQ_TIES[0][0]) == 64 and I.PQ_TIES[1][0] % 64 > I.PQ_TIES[1][1] % 64


class _Recording(Reference):
    """Reference that notes the nodes whose rows a walk reads."""
    def __init__(self, ix):
        super().__init__(ix)
        self.expanded = set()

    def adjacency(self, node):
        self.expanded.add(int(node))
        return super().adjacency(node)


@pytest.mark.parametrize("name", sorted(I.FORM_CASES))
def test_form_queries_find_inserted_points_through_changed_rows(name):
    ix, v, _, _ = I.case(name)
    ix2, st = I.reference(name)
    q = I.form_queries(name)
    assert q.shape[0] == 24
    changed = {int(t) for t in st["targets"]}
    for mode in ("exact", "pq"):
        ref = _Recording(ix2)
        ids, _, _ = ref.search(q, 10, 48, mode)
        found = np.unique(ids[(ids >= ix.N) & (ids < ix2.N)])
        assert len(found) >= 4, (mode, "the answers hold fewer than 4 inserted ids")
        assert ref.expanded & changed, (mode, "the walk expands no old row that the insert changed")
        assert any(x >= ix.N for x in ref.expanded) or mode == "pq"
