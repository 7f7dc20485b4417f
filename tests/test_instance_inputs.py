"""The layout list of tests/instance_inputs.py reaches what it is there for -- asserted ON THE CPU (bang_amd.binding.pq_layout and the other layout
functions run in host code), so that a list that stops reaching an instance fails HERE instead of turning tests/test_gpu_search_instances.py
into a silent pass.  These are conditions, not measurements."""
import ctypes as C

import pytest

import base_forms as F
import edge_inputs as E
import inmemory_reference as M
import instance_inputs as I
from bang_amd import binding as B
from oracle import oracle as O

# The twelve keys (psz * 100 + mp / 4) were read from
#   csrc/bang_search_args.h    BANG_PQ_LAYOUTS, the one list every switch over the layouts is generated from: (1, 8) (1, 16) (1, 24) (1, 32)
#                              (2, 8) (2, 16) (2, 18) (2, 19) (4, 4) (4, 8) (8, 2) (8, 4) as (psz, code dwords); bang_layout_nhi: 58 / 22 for 218 / 219
#   csrc/bang_search.hip       launch_al: ALIGNED from (code_stride ? code_stride : m) % 4
#   csrc/bang_search_host.cpp  bang_pq_layout, bang_ragged_supported
# Whoever adds an instance there extends KEYS here and instance_inputs.ENTRIES.
KEYS = {108, 116, 124, 132, 208, 216, 218, 219, 404, 408, 802, 804}
NHI = {218: 58, 219: 22}

SHAPES = sorted({I.shape_of(e) for e in I.ENTRIES})


def _layout(e):
    ix, _ = I.entry_index(e)
    return B.pq_layout(ix.chunk_off, ix.D, ix.m)


def _supported(libbang, psz, mp, nhi, L):
    libbang.bang_search_supported.argtypes = [C.c_uint32] * 4
    return int(libbang.bang_search_supported(psz, mp, nhi, L))


def test_the_list_is_small_and_mixed():
    assert all(500 <= e.N <= 800 and e.Q <= 12 for e in I.ENTRIES)
    assert {e.R for e in I.ENTRIES} == {8, 32, 64}
    assert {e.dtype for e in I.ENTRIES} == {"uint8", "int8", "float"}
    assert all(e.code_stride == 0 or (e.code_stride % 4 == 0 and e.code_stride >= e.m) for e in I.ENTRIES)     # never -1 (auto)
    assert len({I.entry_id(e) for e in I.ENTRIES}) == len(I.ENTRIES)
    assert {e.key for e in I.ENTRIES if I.has_long_run(e)} == {124, 132, 802, 218}


def test_every_instance_in_both_alignments(libbang):
    for e in I.ENTRIES:
        psz, mp = _layout(e)
        assert psz * 100 + mp // 4 == e.key, I.entry_id(e)
    assert {e.key for e in I.ENTRIES} == KEYS                                      # the twelve keys of search_dispatch, exactly
    for key in KEYS:
        for ragged in ((1, 0) if key in NHI else (1,)):
            al = {I.aligned(e) for e in I.ENTRIES if e.key == key and e.pq_ragged == ragged}
            assert al == {True, False}, (key, ragged)
    assert all(e.pq_ragged == 1 for e in I.ENTRIES if e.key not in NHI)


def test_the_launch_shape_keys_are_in_the_list():
    assert set(I.NEVER_LAUNCHED_BEFORE) <= set(I.LAUNCH_SHAPE_KEYS) <= KEYS


def test_exact_size_table_of_the_70_and_74_chunk_layouts(libbang):
    """pack_pivots_ragged gives the two layouts NHI = 58 / 22; bang_alloc takes the exact-size table where it leaves LDS for more waves than the
    padded one (bang_alloc.cpp: w_rag > w_pad).  74 chunks: at every L of the runs.  70 chunks: not up to L = 37 (both leave room for the 12 waves
    the instance is compiled for) but at L = 152 -- which is why the 218 entries that offer the table have the long run."""
    libbang.bang_ragged_supported.argtypes = [C.c_uint32] * 4
    for e in I.ENTRIES:
        if e.key not in NHI:
            continue
        ix, _ = I.entry_index(e)
        psz, mp = _layout(e)
        nhi, table = B.pack_pivots_ragged(ix.pivots, ix.chunk_off, ix.D, ix.m, mp)
        assert nhi == NHI[e.key] and table is not None
        assert libbang.bang_ragged_supported(psz, mp, nhi, ix.m) == 1
        for _, L in I.runs_of(e):
            w_pad, w_rag = _supported(libbang, psz, mp, 0, L), _supported(libbang, psz, mp, nhi, L)
            assert (w_rag > w_pad) == (e.key == 219 or L == I.LONG_L), (I.entry_id(e), L, w_pad, w_rag)
    assert any(I.has_long_run(e) for e in I.ENTRIES if e.key == 218 and e.pq_ragged and I.aligned(e))
    assert any(I.has_long_run(e) for e in I.ENTRIES if e.key == 218 and e.pq_ragged and not I.aligned(e))


def test_every_run_fits_the_search_kernel(libbang):
    """With the table the entry allows, LDS holds at least the 4 waves below which option search = auto keeps the launch-per-iteration loop
    (bang_alloc.cpp): the GPU tests may assert search_kernel == 1 on every run."""
    for e in I.ENTRIES:
        psz, mp = _layout(e)
        for _, L in I.runs_of(e):
            w = _supported(libbang, psz, mp, 0, L)
            if e.pq_ragged and e.key in NHI:
                w = max(w, _supported(libbang, psz, mp, NHI[e.key], L))
            assert w >= 4, (I.entry_id(e), L, w)


def test_every_run_fits_the_host_paced_form(libbang):
    """... and the host-paced form, which keeps its pacing groups' words in LDS too: a host-paced case of the GPU file that reports
    search_kernel == 0 can only mean device memory the CPU cannot write."""
    for e in I.ENTRIES:
        ix, _ = I.entry_index(e)
        for _, L in I.runs_of(e):
            assert F.host_paced_waves(ix, L, e.pq_ragged) >= 1, (I.entry_id(e), L)


def test_both_rerank_forms_occur(libbang):
    """Layouts the fused re-rank evaluates and layouts that need the re-rank launch, for the never-launched keys too."""
    libbang.bang_search_can_rerank.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32]
    can = {}
    for e in I.ENTRIES:
        ix, _ = I.entry_index(e)
        can.setdefault(e.key, set()).add(libbang.bang_search_can_rerank(O.DTYPE_CODE[e.dtype], e.D, ix.entry_len, 0))
    assert {1, 0} <= set().union(*can.values())
    assert all(can[key] == {0, 1} for key in I.NEVER_LAUNCHED_BEFORE + (132,))
    assert any(e.D % 16 for e in I.ENTRIES if e.dtype != "float")


def test_the_restated_layout_rule_is_the_librarys(libbang):
    """base_forms.fusable makes parameter lists without the library: it answers as bang_search_can_rerank does, on every layout the GPU files run
    and on the strides and dimensions around the rule's edges."""
    libbang.bang_search_can_rerank.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32]
    layouts = {(e.dtype, e.D, e.R) for e in I.ENTRIES} | {(s[2], s[1], s[3]) for s in E.SHAPES} | {(t, D, 64) for t, D in E.TOY_LAYOUTS}
    layouts |= {(t, D, 64) for t in ("uint8", "int8", "float") for D in (1, 3, 4, 15, 16, 17, 48, 96, 250, 256, 260, 272, 512)}
    for dtype, D, R in sorted(layouts):
        for stride in (D * F.tsize(dtype), D * F.tsize(dtype) + 4 + 4 * R):
            assert F.fusable(dtype, D, stride) == bool(libbang.bang_search_can_rerank(O.DTYPE_CODE[dtype], D, stride, 0)), (dtype, D, stride)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-D{s[1]}-{s[2]}-R{s[3]}-m{s[4]}")
def test_the_reference_reaches_the_body_of_the_walk(shape):
    e = next(x for x in I.ENTRIES if I.shape_of(x) == shape)
    ix, q = I.entry_index(e)
    N, D, dtype, R, m, Q = shape
    assert (ix.N, ix.D, ix.dtype, ix.R, ix.m, q.shape) == (N, D, dtype, R, m, (Q, D))
    deg = ix.degrees()
    assert deg.max() == R and deg.min() < R                                        # ragged rows, and some full
    ids, d, st = O.Oracle(ix).search(q, 10, 37, with_stats=True)
    assert not (ids == E.ID_PAD).any()
    assert (st[:, 0] >= 10).all() and (st[:, 0] < 37 + 49).all()                   # past the seed list, and not a walk to the cap
    if R == 64:                                                                    # a full row: 64 ids, no pad, every lane carries one
        ref = M.Reference(ix)
        full = 0
        for i in range(Q):
            _, _, st_i, cand = ref.search_one_logged(q[i], 10, 37, "base")
            assert list(st_i) == st[i].tolist()                                    # the composition walks as the oracle does
            full += int((deg[cand[1:]] == 64).any())                               # (below the cap every logged candidate is expanded)
        assert full >= 1
