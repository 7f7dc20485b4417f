"""Option scan_radix on the GPU (csrc/bang_scan_radix.hip): the exact scan for k up to 4096 by radix select, bit for bit against
tests/scan_reference.py -- large k on every dtype, padded answers, N just above 4096, ragged and second query tiles, any number of runs, ties at the
cut down to the last id digit, masks, the any-dimension layouts with MIPS and the 2^24 hand-over, parity with today's kernels at k <= 128 and the
engine's chunks, times and refusals."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import float_range_inputs as FR
import scan_inputs as SI
import scan_reference as SR
import test_gpu_scan_any as TA

pytestmark = pytest.mark.gpu

KS = (129, 1000, 4096)
NP = {"uint8": np.uint8, "int8": np.int8, "float": np.float32}


def _engine(ix, **opts):
    import bang_amd
    opts.setdefault("graph", bang_amd.GRAPH_DEVICE)
    e = bang_amd.Engine(ix.dtype, **opts)
    e.load_index(ix)
    return e


def _same(got, want, what):
    assert SR.same(got, want), (what, SR.first_difference(got, want))


@functools.lru_cache(maxsize=None)
def _packed(kind):
    """-> (a packed vector table that scan_reference.distances reads as an index, queries [8][D]).
    above: N = 4101 (just above 4096, not a multiple of 32), rows 2050 .. 4099 copies of rows 0 .. 2049: exact duplicates at every cut.
    same:  N = 300, every vector the same: every key differs in its id alone, over two id digits."""
    dtype, N, D = {"above_u8": ("uint8", 4101, 32), "above_f32": ("float", 4101, 5), "same_i8": ("int8", 300, 8), "same_f32": ("float", 300, 3)}[kind]
    rng = np.random.default_rng(7700 + N + D)
    v = rng.integers(0, 64, (N, D)).astype(NP[dtype]) if dtype != "float" else rng.standard_normal((N, D)).astype(np.float32)
    q = rng.integers(0, 64, (8, D)).astype(NP[dtype]) if dtype != "float" else rng.standard_normal((8, D)).astype(np.float32)
    if kind.startswith("above"):
        v[2050:4100] = v[:2050]
    else:
        v[:] = v[0]
    table = np.ascontiguousarray(v).view(np.uint8).reshape(N, -1)
    return types.SimpleNamespace(dtype=dtype, N=N, D=D, entry_len=table.shape[1], graph=table), np.ascontiguousarray(q)


def _k_radix(ix, d_vec, q, k, runs, n_nodes=None):
    """bang_k_scan_radix on device buffers -> ((ids, dists, matched), the keys the emit pass appended per query, the geometry's runs and max_runs)"""
    from bang_amd import binding as B
    lib, Q, n = B.lib(), q.shape[0], ix.N if n_nodes is None else n_nodes
    lib.bang_scan_radix_geometry.argtypes = [C.c_int] + [C.c_uint32] * 4 + [C.c_void_p] * 3
    lib.bang_scan_radix_scratch_bytes.argtypes, lib.bang_scan_radix_scratch_bytes.restype = [C.c_uint32] * 3, C.c_uint64
    t, r, most = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.bang_scan_radix_geometry(B.DTYPE_CODE[ix.dtype], ix.D, Q, n, k, C.byref(t), C.byref(r), C.byref(most)) == 0
    nbytes = int(lib.bang_scan_radix_scratch_bytes(Q, k, max(runs, 1)))
    bufs = dict(q=B.DeviceBuffer.from_numpy(q), scratch=B.DeviceBuffer(nbytes), ids=B.DeviceBuffer(Q * k * 8), dists=B.DeviceBuffer(Q * k * 4),
                matched=B.DeviceBuffer(Q * 4))
    p = B.ScanParams()
    p.d_vec_base, p.vec_stride, p.dtype, p.D, p.n_nodes = d_vec, ix.entry_len, B.DTYPE_CODE[ix.dtype], ix.D, n
    p.d_queries, p.nq, p.k, p.stripes = bufs["q"].ptr, Q, k, runs
    p.d_scratch, p.scratch_bytes, p.d_ids_out, p.d_dists_out, p.d_matched = bufs["scratch"].ptr, nbytes, bufs["ids"].ptr, bufs["dists"].ptr, bufs["matched"].ptr
    lib.bang_k_scan_radix.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.bang_k_scan_radix(C.byref(p), q.shape[1], None) == 0, lib.bang_last_error().decode()
    B.sync()
    got = (bufs["ids"].download(np.uint64, (Q, k)), bufs["dists"].download(np.float32, (k, Q)), bufs["matched"].download(np.uint32, (Q,)))
    words = bufs["scratch"].download(np.uint32, (nbytes // 4,))
    emitted = words[(2 + 256 + 3) * Q:(2 + 256 + 4) * Q]                    # behind prefix u64, bins, rank, fixed, flags: bang_scan_radix_scratch_bytes
    for b in bufs.values():
        b.free()
    return got, emitted, r.value, most.value


@pytest.mark.parametrize("name", ["small_u8", "small_i8", "small_f32"])
def test_large_k_on_every_dtype(request, name):
    """N = 4000 / 2000 / 3000 (the last two no multiple of 32), all below 4096: k = 4096 is padded; one query, and a ragged second tile"""
    ix, q = request.getfixturevalue(name)[:2]
    d0 = SR.distances(ix, q)
    with _engine(ix, scan_radix=1) as e:
        for Q in (1, 33):
            qq, d = SI.queries_of(q, Q), SI.tile_dist(d0, Q)
            for k in KS:
                _same(e.scan(qq, k), SR.answer(d, k), (name, Q, k))
                assert all(v > 0 for v in e.scan_times().values())


@pytest.mark.parametrize("kind,k", [("above_u8", 4096), ("above_f32", 4096), ("above_u8", 129), ("same_i8", 129), ("same_f32", 200)])
def test_any_grid_gives_the_same_buffers(kind, k):
    """runs = 1, the default and the most a launch accepts (one 32-point tile per run): identical outputs, the reference's bits, and the emit pass
    appended exactly min(k, matched) keys.  The duplicated rows / identical vectors tie across the cut: rank k - 1 and rank k are equal distances"""
    from bang_amd import binding as B
    ix, q = _packed(kind)
    d = SR.distances(ix, q)
    qq, dd = SI.queries_of(q, 33), SI.tile_dist(d, 33)
    want = SR.answer(dd, k)
    assert (np.sort(dd, axis=1)[:, k - 1] == np.sort(dd, axis=1)[:, k]).any(), "no query ties at the cut"
    table = B.DeviceBuffer.from_numpy(ix.graph)                              # (exactly N rows: the short last k-step reads nothing behind them)
    try:
        _, _, dflt, most = _k_radix(ix, table.ptr, qq, k, 0)
        assert 1 <= dflt <= most == -(-ix.N // 32)
        for runs in sorted({1, 0, 3, most}):
            got, emitted, _, _ = _k_radix(ix, table.ptr, qq, k, runs)
            _same(got, want, (kind, k, runs))
            assert np.array_equal(emitted, np.minimum(k, got[2])), (kind, k, runs)
        small = _k_radix(ix, table.ptr, qq, k, 0, n_nodes=k - 28)[0]       # a prefix below k: padded
        _same(small, SR.answer(dd, k, n_nodes=k - 28), (kind, k, "n < k"))
    finally:
        table.free()


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_ties_straddle_tiles_and_runs(kind, monkeypatch):
    """50 copies of the nearest vector on ids around every 32-point tile edge, seven runs of one tile each: the lowest ids win at every cut"""
    monkeypatch.setenv("BANG_SCAN_STRIPES", "7")
    ix, q, tied = SI.ties(kind)
    d = SR.distances(ix, q)
    with _engine(ix, scan_radix=2) as e:
        for k in (10, 33, 49, 50, 129):
            assert k >= 50 or (np.sort(d, axis=1)[:, k - 1] == np.sort(d, axis=1)[:, k]).all()
            got = e.scan(q, k)
            _same(got, SR.answer(d, k), (kind, k))
            assert np.array_equal(got[0][:, :min(k, 50)], np.tile(tied[:min(k, 50)], (q.shape[0], 1)))


def test_float_distances_that_are_all_zero():
    ix, q = FR.get("d4", "zero")
    d = SR.distances(ix, q)
    assert (d.view(np.uint32) == 0).all()
    with _engine(ix, scan_radix=1) as e:
        for k in (129, 600, 1000):
            _same(e.scan(q, k), SR.answer(d, k), k)


@pytest.mark.parametrize("name", ["small_u8", "small_f32"])
def test_masks(request, name):
    """an exclusion set, a removed set and filters that leave a tile's queries with every candidate, three candidates (< k) and none"""
    ix, q = request.getfixturevalue(name)[:2]
    d0, x = SR.distances(ix, q), SI.excl_edges(ix.N)
    qq, d = SI.queries_of(q, 33), SI.tile_dist(d0, 33)
    lab = np.random.default_rng(9300).integers(0, 16, ix.N).astype(np.uint32)
    lab[[5, 130, ix.N - 2]] |= 0x100
    a = np.array([0, 1, 0x100, 0x200, 3, 0, 0x100, 6], np.uint32)[np.arange(33) % 8]
    b = np.array([0, 0, 0, 0, 1, 2, 0x100, 4], np.uint32)[np.arange(33) % 8]
    with _engine(ix, capacity=ix.N, scan_radix=1) as e:
        e.set_labels(lab)
        e.set_excluded(x)
        for k in (129, 1000):
            got = e.scan(qq, k, a, b)
            _same(got, SR.answer(d, k, excluded=x, labels=lab, any_=a, all_=b), (name, k, "excluded, filters"))
        assert (got[2][2::8] == 3).all() and (got[2][3::8] == 0).all() and (got[2][0::8] == ix.N - len(x)).all()
        e.consolidate(1.2)                                                 # X \ {medoid} is removed, X & {medoid} stays excluded: the same candidates
        _same(e.scan(qq, 1000), SR.answer(d, 1000, excluded=x), (name, "removed"))
        e.clear_excluded()
        gone = x[x != ix.medoid]
        _same(e.scan(qq, 129, a, b), SR.answer(d, 129, removed=gone, labels=lab, any_=a, all_=b), (name, "removed, filters"))


@pytest.mark.parametrize("name", ["i8_100", "f32_67", "f32_201_mips", "u8_20_mips", "i8_1020_far", "handover"])
def test_any_dimension_layouts_without_scan_any(name):
    """a short last k-step, an odd float D, MIPS queries of D - 1 elements, and the widest 8-bit rows with extreme bytes: every sum of i8_1020_far
    is beyond 2^24, handover's lie on both sides -- the chain's value, not the integer's float image"""
    ix, q = TA._get(name)
    d = TA._dist(name)
    if name in ("i8_1020_far", "handover"):
        assert d.max() > 2.0 ** 24 and ix.D >= 1020
    with TA._engine(name, scan_any=0, scan_radix=1) as e:
        for k in (10, 129, 300):                                           # 10: routed here because today's kernels refuse the layout
            _same(e.scan(q, k), SR.answer(d, k), (name, k))


@pytest.mark.parametrize("name", SI.FIXTURES)
def test_small_k_equals_todays_kernels(request, name):
    ix, q = request.getfixturevalue(name)[:2]
    with _engine(ix) as e:
        for k in (1, 10, 128):
            e.set_option("scan_radix", 0)
            want = e.scan(q, k)
            e.set_option("scan_radix", 2)
            _same(e.scan(q, k), want, (name, k))


def test_engine_chunks_and_refusals(small_i8, small_f32, monkeypatch):
    import bang_amd
    ix, q = small_i8[:2]
    d = SR.distances(ix, q)
    monkeypatch.setenv("BANG_SCAN_QUERY_CHUNK", "5")                         # 32 queries in seven launches, the last of two
    with _engine(ix, scan_radix=1) as e:
        _same(e.scan(q, 1000), SR.answer(d, 1000), "chunks")
        assert all(v > 0 for v in e.scan_times().values())
        TA._raw_refused(e, q, 4097, -1, "k = 4097")
        _same(e.scan(q, 129), SR.answer(d, 129), "after the refusal")
        e.set_option("scan_radix", 0)
        TA._raw_refused(e, q, 129, -1, "k = 129")                          # the option at 0: refused as ever
    ix, q = small_f32[:2]
    with _engine(ix, graph=bang_amd.GRAPH_HOST, pull=1, vectors_fp16=1, scan_radix=1) as e:
        TA._raw_refused(e, q, 1000, -5, "fp16")
