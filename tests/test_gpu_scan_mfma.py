"""Option scan_mfma of the exact scan (csrc/bang_scan_mfma.hip): the fp32 MFMA prefilter with its exact refine against
tests/scan_reference.py, bit for bit -- layouts, the ends of the float range, near ties at the threshold, masks -- and what the counters say."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import float_range_inputs as FR
import scan_reference as SR
import test_gpu_scan_any as TA
from bang_amd import synth
from bang_amd.formats import pack_graph

pytestmark = pytest.mark.gpu

LAYOUTS = ("f32_5", "f32_67", "f32_201_mips", "f32_257", "f32_1023", "f32_96_mips", "f32_960")
N_TIES = 48


def _scan(ix, q, k, *filt, **opts):
    with TA._engine("", ix, scan_mfma=1, **opts) as e:
        return e.scan(q, k, *filt), e.scan_counters()


@pytest.mark.parametrize("stripes", [1, 3])
@pytest.mark.parametrize("name", LAYOUTS + ("small_f32",))
def test_every_layout_at_every_k(name, stripes, monkeypatch, small_f32):
    monkeypatch.setenv("BANG_SCAN_STRIPES", str(stripes))
    if name == "small_f32":                                    # a narrow layout, without scan_any
        ix, q = small_f32[:2]
        e, d = TA._engine("", ix, scan_any=0, scan_mfma=1), SR.distances(ix, q)
    else:
        q, e, d = TA._get(name)[1], TA._engine(name, scan_mfma=1), TA._dist(name)
    with e:
        for k in (1, 10, 128):
            TA._same(e.scan(q, k), SR.answer(d, k), (name, stripes, k))
            assert e.scan_counters()["tested"] == d.size and 0 < e.scan_counters()["refined"] <= d.size


@pytest.mark.parametrize("what", FR.NAMES)
def test_the_ends_of_the_float_range(what):
    ix, q = FR.get("d68", what)
    got, n = _scan(ix, q, 10)
    TA._same(got, SR.answer(SR.distances(ix, q), 10), what)
    if what == "offset":                                       # the bound exceeds every distance: nothing can be discarded
        assert n["refined"] == n["tested"] == q.shape[0] * ix.N


@functools.lru_cache(maxsize=None)
def _ties():
    """300 points at D = 68: N_TIES of them are one vector, 16 bit for bit and the others with the last mantissa bit of one coordinate flipped;
    the queries stand next to that vector"""
    ix, q, _, _ = synth.make_index(300, 68, "float", 16, 17, 8, K=10, n_clusters=4, seed=9300, device="cpu", pq_iters=1)
    rng = np.random.default_rng(9301)
    v = np.array(ix.vectors(), np.float32)
    ids = np.sort(rng.choice(300, N_TIES, replace=False))
    v[ids] = v[ids[0]]
    for j, x in enumerate(ids[16:]):
        v[x, j % 68:j % 68 + 1].view(np.uint32)[0] ^= 1
    q = (v[ids[0]][None, :] + rng.normal(0, 0.01, q.shape)).astype(np.float32)
    return dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency())), np.ascontiguousarray(q)


@pytest.mark.parametrize("k", [10, 30])
def test_near_ties_at_the_threshold(k):
    ix, q = _ties()
    d = SR.distances(ix, q)
    s = np.sort(d, axis=1)
    assert (s[:, k - 1] == s[:, k]).any() and (s[:, N_TIES - 1] < s[:, N_TIES] / 4).all(), "the input has no tie across rank k"
    TA._same(_scan(ix, q, k)[0], SR.answer(d, k), k)


def test_masks():
    name = "f32_201_mips"
    ix, q = TA._get(name)
    d, x = TA._dist(name), np.array([0, 31, 32, ix.N - 1], np.uint32)
    lab = np.random.default_rng(9200).integers(0, 16, ix.N).astype(np.uint32)
    lab[[5, 130, 290]] |= 0x100                                # three nodes: a filter on bit 8 matches fewer than k
    a = np.array([0, 1, 3, 0x100, 0, 6, 0x100, 15], np.uint32)
    b = np.array([0, 0, 1, 0, 2, 4, 0x100, 0], np.uint32)
    with TA._engine(name, scan_mfma=1) as e:
        e.set_excluded(x)
        TA._same(e.scan(q, 10), SR.answer(d, 10, excluded=x), "excluded")
        assert e.scan_counters()["tested"] == q.shape[0] * (ix.N - len(x))
        e.set_labels(lab)
        want = SR.answer(d, 10, excluded=x, labels=lab, any_=a, all_=b)
        TA._same(e.scan(q, 10, a, b), want, "excluded, filters")
        assert e.scan_counters()["tested"] == int(want[2].sum())


def test_a_packed_table_that_ends_its_buffer():
    """host placement on a caller's vector buffer of exactly N rows, D = 1023: neither the products nor the refine touch a byte behind the last row"""
    import bang_amd
    from bang_amd import binding as B
    ix, q = TA._get("f32_1023")
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)
    source = lambda first, count, dst: C.memmove(dst, graph[first:first + count].ctypes.data, count * ix.entry_len) and 0    # noqa: E731
    buf = B.DeviceBuffer(ix.N * ix.D * 4)
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1, distance=bang_amd.DISTANCE_EXACT, any_dim=1, scan_any=1, scan_mfma=1) as e:
        e.load_stream(ix, source, d_vectors=buf.ptr)
        for k in (10, 128):
            TA._same(e.scan(q, k), SR.answer(TA._dist("f32_1023"), k), k)


def test_the_prefilter_prunes_and_the_option_changes_no_bit(small_f32, monkeypatch):
    ix, q = small_f32[:2]
    monkeypatch.setenv("BANG_SCAN_STRIPES", "1")
    got, n = _scan(ix, q, 10, scan_any=0)
    TA._same(got, SR.answer(SR.distances(ix, q), 10), "k = 10")
    assert n["tested"] == q.shape[0] * ix.N and n["refined"] < n["tested"] // 2, n
    monkeypatch.delenv("BANG_SCAN_STRIPES")
    with TA._engine("", ix, scan_any=0) as e:
        off = e.scan(q, 100)
        assert e.scan_counters() == dict(tested=0, refined=0)
        e.set_option("scan_mfma", 1)                           # settable at any time
        TA._same(e.scan(q, 100), off, "scan_mfma = 1 against 0")
        assert e.scan_counters()["tested"] == q.shape[0] * ix.N
