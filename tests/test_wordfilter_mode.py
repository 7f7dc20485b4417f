"""The word-local visited filter (option "filter_layout" = 1) -- what can be checked without a GPU: the CPU reference the GPU tests compare
against (tests/wordfilter_reference.py) and the crafted inputs that make those comparisons mean something (tests/wordfilter_inputs.py)."""
import numpy as np
import pytest

import wordfilter_inputs as WI
import wordfilter_reference as W

K = 10


@pytest.mark.parametrize("fixture,L,nq", [("small_u8", 10, 16), ("small_u8", 37, 8), ("small_f32", 10, 16), ("small_f32", 37, 8)])
def test_split_composition_is_the_oracle(request, fixture, L, nq):
    """The reference loop with filter = split equals Oracle.search bit for bit, counters included: what the `word` layout changes is the filter
    stage and nothing else."""
    from oracle import oracle as O
    ix, q, _, _ = request.getfixturevalue(fixture)
    q = q[:nq]
    ids, d, st = W.Reference(ix).search(q, K, L, "split")
    ids_o, d_o, st_o = O.Oracle(ix).search(q, K, L, with_stats=True)
    assert np.array_equal(ids, ids_o)
    assert np.array_equal(d.view(np.uint32), d_o.view(np.uint32))
    assert np.array_equal(st, st_o)


def test_split_composition_is_the_oracle_with_mips(small_f32):
    from oracle import oracle as O
    ix, q, _, _ = small_f32
    q1 = np.ascontiguousarray(q[:8, :-1])
    ids, d, _ = W.Reference(ix).search(q1, K, 24, "split", mips=True)
    ids_o, d_o = O.Oracle(ix).search(q1, K, 24, mips=True)
    assert np.array_equal(ids, ids_o)
    assert np.array_equal(d.view(np.uint32), d_o.view(np.uint32))


@pytest.mark.parametrize("fixture", ["small_u8", "small_f32"])
def test_layouts_agree_on_the_plain_fixtures(request, fixture):
    """On an ordinary small index a query sets a few hundred of 400 384 bits and neither layout drops an id it has not seen: the two references
    agree in everything.  THIS is why tests/wordfilter_inputs.py exists -- on these fixtures a kernel that ignored the option would pass."""
    ix, q, _, _ = request.getfixturevalue(fixture)
    ref = W.Reference(ix)
    a, b = ref.search(q[:12], K, 24, "split"), ref.search(q[:12], K, 24, "word")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def test_word_rule_on_hand_made_ids():
    """The rule of DESIGN.md section 2 row 16 on the colliding ids themselves: snapshot, "dropped only if all bits are set", input order, two
    survivors of one row sharing a word, a one-bit mask."""
    c = WI.collisions()
    a, x = c.word_only[0]
    words = np.zeros(W.BF_WORDS, np.uint32)
    assert W.filter_word(words, [a, x, a]).tolist() == [a, x, a]            # one row: everything is tested against the state at entry
    assert W.filter_word(words, [x, a]).tolist() == []                      # both known now
    words[:] = 0
    assert W.filter_word(words, [a]).tolist() == [a] and W.filter_word(words, [x]).tolist() == []       # x's mask lies inside a's
    u, v, w = c.shared_word[0]
    words[:] = 0
    assert W.filter_word(words, [u]).tolist() == [u] and W.filter_word(words, [w]).tolist() == [w]       # u alone does not cover w
    words[:] = 0
    assert W.filter_word(words, [v, u]).tolist() == [v, u]                  # input order kept; both masks land in the shared word
    assert int(words[W.word_of(u)]) == W.mask_of(u) | W.mask_of(v)
    assert W.filter_word(words, [w]).tolist() == []
    z = c.one_bit[0]
    a1, b1 = W.positions(z)
    assert (a1 & 31) == ((b1 >> 5) & 31) and W.mask_of(z) == 1 << (a1 & 31)
    words[:] = 0
    assert W.filter_word(words, [z]).tolist() == [z] and int(words[W.word_of(z)]) == W.mask_of(z) and W.filter_word(words, [z]).tolist() == []
    for x in (a, u, z, 8191):                                               # position b stays in the word of position a
        h1, h2 = W.positions(x)
        b = (h1 & ~31) | ((h2 >> 5) & 31)
        assert b >> 5 == h1 >> 5 == W.word_of(x) < W.BF_WORDS and W.mask_of(x) == (1 << (h1 & 31)) | (1 << (b & 31))


def test_collisions_come_from_the_oracle_hashes():
    """Every kind of collision exists below N = 8192 (the search raises otherwise) and each listed tuple has the property its kind claims."""
    c = WI.collisions()
    for a, x in c.word_only:
        assert W.word_of(a) == W.word_of(x) and W.mask_of(x) & ~W.mask_of(a) == 0
        assert not set(W.positions(x)) <= set(W.positions(a))
    for a1, a2, x in c.split_only:
        assert W.positions(x)[0] in W.positions(a1) and W.positions(x)[1] in W.positions(a2)
    for u, v, w in c.shared_word:
        assert W.word_of(u) == W.word_of(v) == W.word_of(w)
    assert len(c.one_bit) > 100                                             # about 1 id in 32


@pytest.mark.parametrize("name", list(WI.INPUTS))
def test_crafted_input_parts_the_layouts(name):
    """On each crafted input the stated id is offered to the filter in the stated iteration of the stated query, dropped there by one layout and
    evaluated by the other -- and so dist_evals and the results (or the candidate log) of the two references differ."""
    inp = WI.INPUTS[name]()
    assert inp.ix.N <= 8192 and inp.ix.D == 32 and inp.q.shape[0] <= 70
    ref = W.Reference(inp.ix)
    out, logs = {}, {}
    for layout in W.LAYOUTS:
        trace, logs[layout] = [], []
        out[layout] = ref.search_one(inp.q[inp.query], K, WI.L_TRACE, layout, trace=trace, log=logs[layout])
        offered, kept = [(t, s) for it, t, s in trace if it == inp.iteration][0]
        assert inp.id in offered
        assert (inp.id in kept) == (layout != inp.dropped_by), (layout, inp)
    assert out["split"][2][2] != out["word"][2][2]                          # dist_evals
    assert logs["split"] != logs["word"] or not np.array_equal(out["split"][0], out["word"][0])


def test_seed65_has_the_65_id_seed_list():
    inp = WI.seed65()
    ref = W.Reference(inp.ix)
    row = ref.adjacency(int(inp.ix.medoid))
    u, v, w = WI.collisions().shared_word[0]
    assert len(row) == 64 and inp.ix.R == 64 and int(row[-1]) == v and u in row and inp.id == w
    trace = []
    ref.search_one(inp.q[inp.query], K, WI.L_TRACE, "word", trace=trace)
    assert len(trace[0][1]) == 65 and len(trace[0][2]) == 65                # all 65 survive iteration 1, the two that share a word included


def test_shared_word_row_holds_two_fresh_ids_of_one_word():
    inp = WI.shared_word_row()
    u, v, w = WI.collisions().shared_word[0]
    trace = []
    W.Reference(inp.ix).search_one(inp.q[inp.query], K, WI.L_TRACE, "word", trace=trace)
    offered, kept = [(t, s) for it, t, s in trace if it == 2][0]
    assert u in offered and v in offered and u in kept and v in kept and W.word_of(u) == W.word_of(v)
