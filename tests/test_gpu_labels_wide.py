"""Label filters on the wide vector layouts (Engine(labels_wide=1): bang_k_search_exact_labels_wide, search_exact_wide_labels[_pull]_kernel) on a
GPU, bit for bit against tests/labels_reference.py over tests/exact_reference.py: ids, distance bits, matched counts, the walk's counters and the
candidate log.  Every batch mixes unfiltered queries with any-only, all-only and any + all filters on a bit half the points carry, a bit 1 % carry
and a bit nobody carries, first without and then with a few excluded ids."""
import functools

import numpy as np
import pytest

import highdim_inputs as H
import labels_reference as LR
import launch_shapes as S

pytestmark = pytest.mark.gpu

FORMS = {"hbm": dict(graph=1, distance=1), "pull": dict(graph=0, pull=1, distance=1)}
# u8_48: D / 16 = 3, the smallest wide 8-bit row; u8_192: the YFCC shape; i8_1024: far_i8, every chain crosses the 2^24 hand-over, the largest
# tile; f32_260: the smallest wide float row; f32_1024: the LDS maximum
LAYOUTS = ("u8_48", "u8_192", "i8_1024", "f32_260", "f32_1024")
HALF, RARE, NONE = 1, 2, 4                                             # label bits: about half the points, about 1 %, nobody
FILTERS = ((0, 0), (HALF, 0), (0, HALF), (RARE, 0), (HALF | RARE, HALF), (NONE, 0), (0, RARE), (HALF, NONE))     # (any, all) by query position


@functools.lru_cache(maxsize=None)
def _input(name):
    """-> (index, queries, labels)"""
    from bang_amd import synth
    if name == "u8_192":
        ix, q = synth.make_index(1500, 192, "uint8", 32, 48, 16, K=10, n_clusters=8, seed=192, device="cpu", pq_iters=2)[:2]
    elif name == "f32_1024":
        ix, q = synth.make_index(1000, 1024, "float", 24, 64, 16, K=10, n_clusters=8, seed=1024, device="cpu", pq_iters=2)[:2]
    else:
        ix, q = H.get("far_i8" if name == "i8_1024" else name)
    rng = np.random.default_rng(ix.N)
    labels = (rng.random(ix.N) < 0.5) * np.uint32(HALF) | (rng.random(ix.N) < 0.01) * np.uint32(RARE)
    return ix, np.ascontiguousarray(q), labels.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _traces(name, L):
    return LR.Reference(_input(name)[0]).walks(_input(name)[1], L)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(e, q, k, L, filters=None):
    """-> ids, dists, counters, log, log counts, matched, stats"""
    Q = q.shape[0]
    e.set_searchparams(k, L)
    e.alloc(Q)
    if filters is not None:
        e.set_filters(*filters)
    e.init(Q)
    out = e.query(q) + (e.query_counters(Q),) + e.candidate_log(Q, L) + (e.matched_counts(Q) if filters is not None else None, e.stats())
    e.free()
    return out


def _case(name, form, k, L, Q):
    import bang_amd
    ix, q0, labels = _input(name)
    pick = [i % len(q0) for i in range(Q)]                                 # (a batch longer than the input repeats its queries, under other filters)
    q, tr = np.ascontiguousarray(q0[pick]), [_traces(name, L)[i] for i in pick]
    any_, all_ = (np.array([FILTERS[(i + i // len(q0)) % len(FILTERS)][j] for i in range(Q)], np.uint32) for j in (0, 1))
    plain = (any_ | all_) == 0
    with bang_amd.Engine(ix.dtype, **FORMS[form]) as e:
        e.load_index(ix)
        e.set_labels(labels)
        e.set_searchparams(k, L)
        e.alloc(Q)
        with pytest.raises(bang_amd.BangError, match="filters on labels are not available on the wide vector layouts"):      # labels_wide = 0: as ever
            e.set_filters(any_, all_)
        e.free()
        e.set_option("labels_wide", 1)
        base = _run(e, q, k, L)                                            # no filters: today's launch on the wide instance
        for ex in (None, np.unique(np.concatenate([t.wl_ids[:2] for t in tr[:4]]))):      # ... then without ids that the answers would hold
            if ex is not None:
                e.set_excluded(ex)
            got = _run(e, q, k, L, (any_, all_))
            ids, d, matched, st, _ = LR.collect_all(tr, labels, any_, all_, k, L, int(ix.medoid), ex)
            assert np.array_equal(got[0], ids) and np.array_equal(_bits(got[1]), _bits(d)), ex
            assert np.array_equal(got[5], matched) and matched[any_ == NONE].sum() == 0 and matched.any(), ex
            assert np.array_equal(got[2], st) and np.array_equal(got[2], base[2]) and np.array_equal(got[4], base[4]), ex      # the walk is untouched
            assert all(np.array_equal(got[3][i, :got[4][i]], t.log) and np.array_equal(base[3][i, :base[4][i]], t.log) for i, t in enumerate(tr)), ex
            assert got[6]["label_launches"] == 1 and got[6]["exclude_launches"] == 0 and base[6]["label_launches"] == 0, got[6]
            if ex is None:                                                 # an unfiltered query of a filtered batch: the unfiltered engine's answer
                assert plain.any() and np.array_equal(got[0][plain], base[0][plain]) and np.array_equal(_bits(got[1][:, plain]), _bits(base[1][:, plain]))
                assert not np.array_equal(got[0], base[0])
        e.unload()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", LAYOUTS)
def test_filtered_walks(name, form):
    _case(name, form, 10, 37, 16)


@pytest.mark.parametrize("shape", ("one_workgroup", "ragged"))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ("u8_192", "i8_1024", "f32_1024"))
def test_long_lists_in_full_workgroups(monkeypatch, name, form, shape):
    """L = k = 512: waves side by side in LDS, and a second query for a wave (the caps of tests/launch_shapes.py)"""
    S.set_caps(monkeypatch, shape)
    _case(name, form, S.MAX_L, S.MAX_L, S.NQ)
