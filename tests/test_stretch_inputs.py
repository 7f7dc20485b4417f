"""tests/stretch_inputs.py on the CPU references alone: the stretched tables of tests/test_gpu_offsets64.py are not vacuous.  For every (input,
table, mode) a GPU case uses -- the list is made from the same CASES -- at least a quarter of the rows the reference walk reads lie beyond 4 GiB
of the stretched table and at least one beyond 16 GiB, and the reference on the index a kernel would see if it wrapped that table's offsets at
2^32 or 2^34 differs from the reference on the index in ids or distance bits: such a kernel cannot pass the GPU comparison.  These are
conditions on the inputs; an input that misses them is changed, not the bound."""
import numpy as np
import pytest

import stretch_inputs as S

PARAMS = S.cpu_params()
_REF = {}


def _ref(name, mode):
    if (name, mode) not in _REF:
        _REF[(name, mode)] = S.reference(*S.get(name), mode)
    return _REF[(name, mode)]


def _beyond(ids, stride):
    off = np.asarray(ids, np.int64) * stride
    return float((off >= 4 * S.GIB).mean()), int((off >= 16 * S.GIB).sum())


# ------------------------------------------------------------------------------------------------------------------------ the helpers themselves
def test_strides_keep_the_alignment_class_and_reach_both_marks():
    for c in S.CASES:
        for which in c.tables:
            stride, compact = S.stride_for(c, which), S.stride_for(c, which) - S.BLOW
            assert stride % 16 == compact % 16 and stride < 2**32                    # (code_stride is a 32-bit argument)
            assert 127 * stride < 4 * S.GIB <= 128 * stride and 511 * stride < 16 * S.GIB <= 512 * stride
            assert S.LEAD + S.SHARE_GAP + S.N * stride + 256 <= 24 * S.GIB           # what a test may hold
    assert S.LEAD >= 2**31                                                           # a sign-extended 32-bit offset stays inside the buffer


def test_wrapped_table_reads_the_stretched_image():
    rng = np.random.default_rng(1)
    t = rng.integers(1, 256, (40, 24)).astype(np.uint8)
    stride, bits = 1001, 10                                                          # a small image, built in full
    image = np.zeros(40 * stride + 64, np.uint8)
    for i in range(40):
        image[i * stride: i * stride + 24] = t[i]
    w = S.wrapped_table(t, stride, bits)
    for i in range(40):
        o = (i * stride) % (1 << bits)
        assert np.array_equal(w[i], image[o:o + 24]), i
    assert np.array_equal(w[:2], t[:2])                                              # two rows begin below 2^10
    assert w[2, -1] == t[1, 0] and not w[2, :-1].any()                               # offset 978: a shifted piece of row 1, which begins at 1001
    assert not w[3].any()                                                            # offset 955: no row lies there
    big = S.wrapped_table(t, S.stride_of(24), 32)                                    # the strides of the cases: rows >= 128 would read zeros
    assert np.array_equal(big, t)


def test_wrapped_index_changes_one_table_only():
    ix, _ = S.get("u8_128_m70")
    for which in ("graph", "vectors", "codes"):
        stride = S.stride_of(S.compact_stride("u8_128_m70", which))
        for bits, first in ((32, 128), (34, 512)):
            w = S.wrapped(ix, which, stride, bits)
            assert np.array_equal(w.codes, ix.codes) == (which != "codes")
            assert np.array_equal(w.adjacency(), ix.adjacency()) == (which != "graph")
            assert np.array_equal(w.vectors(), ix.vectors()) == (which == "codes")
            changed = w.codes if which == "codes" else w.graph[:, :128] if which == "vectors" else w.graph
            same = ix.codes if which == "codes" else ix.graph[:, :128] if which == "vectors" else ix.graph
            assert np.array_equal(changed[:first], same[:first]) and not changed[first:].any()


@pytest.mark.parametrize("name", sorted({c.input for c in S.CASES if c.mode == "base"}))
def test_logged_base_walk_is_the_oracles(name):
    """walk() takes the base walk's log from wordfilter_reference's split layout: its results and counters are Oracle.search's."""
    w, ref = S.walk(name, "base"), _ref(name, "base")
    assert not S.differs(w, ref) and np.array_equal(w.stats, ref[2])
    assert [len(x) for x in w.logs] == list(ref[2][:, 1])


# ------------------------------------------------------------------------------------------------------------------------ the two conditions
@pytest.mark.parametrize("name,which,mode,stride,fp16", PARAMS, ids=lambda v: str(v))
def test_reference_walk_reads_beyond_both_marks(name, which, mode, stride, fp16):
    w = S.walk(name, mode)
    read = {"codes": w.codes, "vectors": w.vectors, "graph": np.concatenate(w.logs).astype(np.int64)}[which]
    assert len(read) > 0
    share, far = _beyond(read, stride)
    assert share >= 0.25 and far >= 1, (share, far)
    if which == "graph":                                                             # the log is what the walk expanded
        assert set(w.graph) <= set(read)
    ref = _ref(name, mode)                                                           # walk() restates the mode's reference query by query
    assert not S.differs(w, ref) and np.array_equal(w.stats, ref[2])


@pytest.mark.parametrize("bits", S.WRAPS)
@pytest.mark.parametrize("name,which,mode,stride,fp16", PARAMS, ids=lambda v: str(v))
def test_a_wrapped_offset_changes_the_answer(name, which, mode, stride, fp16, bits):
    ix, q = S.get(name)
    assert S.differs(S.reference(S.wrapped(ix, which, stride, bits, fp16=fp16), q, mode), _ref(name, mode))


# ------------------------------------------------------------------------------------------------------------------------ the entries without a walk
def test_pqdist_lists_and_vector_logs_reach_both_marks():
    """bang_k_pqdist_stream's neighbour lists, the slots of the vector logs of bang_k_rerank's two host-graph forms, and the 640 rows of the
    fp16 conversion: the same two conditions on what tests/test_gpu_offsets64.py hands those entries."""
    name = "u8_128_m70"
    ix, q = S.get(name)
    from oracle import oracle as O
    orc = O.Oracle(ix)
    lists = S.pqdist_lists()
    share, far = _beyond(np.concatenate(lists), S.stride_of(ix.m))
    assert share >= 0.25 and far >= 1
    for bits in S.WRAPS:
        worc = O.Oracle(S.wrapped(ix, "codes", S.stride_of(ix.m), bits))
        assert any(not np.array_equal(orc.pqdist(orc.lut_build(q[i]), l).view(np.uint32), worc.pqdist(worc.lut_build(q[i]), l).view(np.uint32))
                   for i, l in enumerate(lists))
    for name in ("u8_128_m70", "f32_96_m74"):
        ix, q = S.get(name)
        w = S.walk(name, "base")
        for form in ("by_row", "by_query"):
            slots, stride = S.log_slots(w.logs, form), S.log_stride(ix)
            used = np.concatenate(slots)
            assert len(set(used)) == len(used)                                       # every candidate has a slot of its own
            share, far = _beyond(used, stride)
            assert share >= 0.25 and far >= 1, (form, share, far)
            assert (used.max() + 1) * stride + S.LEAD + 256 <= 24 * S.GIB
            table = np.zeros((int(used.max()) + 1, ix.D * S.tsize(ix)), np.uint8)
            for i, log in enumerate(w.logs):
                table[slots[i]] = ix.graph[log[1:].astype(np.int64), :table.shape[1]]
            want = S.rerank_of_slots(ix, q, w.logs, slots, table)
            assert not S.differs(want, _ref(name, "base"))                           # the re-rank of the log IS the search's result
            for bits in S.WRAPS:
                assert S.differs(S.rerank_of_slots(ix, q, w.logs, slots, S.wrapped_table(table, stride, bits)), want)
    for D in S.CONVERT_D:
        src = S.convert_rows(D)
        assert src.shape[0] == S.N and src[128:].all() and src[512:].all()           # a row written to a wrapped place leaves zeros where it belongs
        with np.errstate(over="ignore"):
            want = src.astype(np.float16)
        assert (want[128:].view(np.uint16) & 0x7FFF).any(axis=1).all()
        for bits in S.WRAPS:
            got = S.wrapped_table(src, S.stride_of(4 * D), bits).view(np.float32).astype(np.float16)
            assert not np.array_equal(got.view(np.uint16), want.view(np.uint16))
