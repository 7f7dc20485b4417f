"""Option scan_any of the exact scan (csrc/bang_scan_any.hip; DESIGN.md section 2 CANON 25): every any-dimension layout of tests/anydim_inputs.py and
three wide ones against tests/scan_reference.py bit for bit, the 2^24 hand-over of the 8-bit kernel, masks, a packed table that ends its buffer, the
default and the refusals."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import anydim_inputs as A
import scan_reference as SR
from bang_amd import synth
from bang_amd.formats import pack_graph
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WIDE = {"u8_48": (48, "uint8"), "u8_784": (784, "uint8"), "f32_960": (960, "float")}       # name -> (D, dtype), N = 300
HAND_NEAR = (0, 31, 32, 100, 127, 128, 200, 255, 256, 299)                                  # the ten points of "handover" whose sums stay far below 2^24


@functools.lru_cache(maxsize=None)
def _get(name):
    """-> (Index, queries [8][D or D - 1])"""
    if name in A.TABLE:
        return A.get(name)
    D, dtype = (1024, "uint8") if name == "handover" else WIDE[name]
    ix, q, _, _ = synth.make_index(300, D, dtype, 16, D // 4, A.Q, K=10, n_clusters=4, seed=9000 + D, device="cpu", pq_iters=1)
    if name == "handover":                                     # built as anydim_inputs builds i8_1020_far: the vectors replaced, the rows kept
        rng = np.random.default_rng(9100)
        v = rng.integers(248, 256, (300, D)).astype(np.uint8)
        v[list(HAND_NEAR)] = rng.integers(0, 8, (len(HAND_NEAR), D)).astype(np.uint8)
        q = rng.integers(0, 8, q.shape).astype(np.uint8)
        ix = dataclasses.replace(ix, graph=pack_graph(v, ix.degrees(), ix.adjacency()))
    return ix, np.ascontiguousarray(q)


@functools.lru_cache(maxsize=None)
def _dist(name):
    """float32 [Q][N] of orc_exact_dist; MIPS: the same loop as scan_reference.distances with dim_adjust = 1"""
    ix, q = _get(name)
    if not A.is_mips(name):
        return SR.distances(ix, q)
    fn, g = O.lib().orc_exact_dist, np.ascontiguousarray(ix.graph, dtype=np.uint8)
    D, code, one = C.c_uint32(ix.D), C.c_int(O.DTYPE_CODE[ix.dtype]), C.c_int(1)
    return np.array([[fn(C.c_void_p(g.ctypes.data + x * int(ix.entry_len)), C.c_void_p(qi.ctypes.data), D, code, one) for x in range(int(ix.N))]
                     for qi in q], np.float32)


def _engine(name, ix=None, scan_any=1, **opts):
    import bang_amd
    ix = _get(name)[0] if ix is None else ix
    opts.setdefault("graph", bang_amd.GRAPH_DEVICE)
    e = bang_amd.Engine(ix.dtype, scan_any=scan_any, **opts)
    e.load_index(ix)
    if A.is_mips(name):
        e.set_searchparams(10, 37, bang_amd.DIST_MIPS)
    return e


def _same(got, want, what):
    assert SR.same(got, want), (what, SR.first_difference(got, want))


@pytest.mark.parametrize("stripes", [1, 3])
@pytest.mark.parametrize("name", A.NAMES + tuple(WIDE))
def test_every_layout_at_every_k(name, stripes, monkeypatch):
    monkeypatch.setenv("BANG_SCAN_STRIPES", str(stripes))
    _, q = _get(name)
    with _engine(name) as e:
        for k in (1, 10, 128):
            _same(e.scan(q, k), SR.answer(_dist(name), k), (name, stripes, k))


@pytest.mark.parametrize("k", [10, 100])
def test_sums_on_both_sides_of_2_pow_24(k):
    """ten points far below 2^24, 290 near 5.9e7: at k = 100 the answer holds distances that are NOT float32(integer sum)"""
    ix, q = _get("handover")
    want = SR.answer(_dist("handover"), 100)
    v, qq = ix.vectors().astype(np.int64), q.astype(np.int64)
    plain = np.array([[((v[int(x)] - qq[i]) ** 2).sum() for x in want[0][i]] for i in range(q.shape[0])], np.int64).astype(np.float32)
    assert (plain.view(np.uint32) != np.ascontiguousarray(want[1].T).view(np.uint32)).any(), "the input does not tell the chain from the integer's float image"
    with _engine("handover") as e:
        _same(e.scan(q, k), SR.answer(_dist("handover"), k), k)


@pytest.mark.parametrize("name", ["u8_784", "f32_201_mips"])
def test_masks_on_a_wide_layout(name):
    ix, q = _get(name)
    d, x = _dist(name), np.array([0, 31, 32, ix.N - 1], np.uint32)
    lab = np.random.default_rng(9200).integers(0, 16, ix.N).astype(np.uint32)
    lab[[5, 130, 290]] |= 0x100                                # three nodes: a filter on bit 8 matches fewer than k
    a = np.array([0, 1, 3, 0x100, 0, 6, 0x100, 15], np.uint32)
    b = np.array([0, 0, 1, 0, 2, 4, 0x100, 0], np.uint32)
    with _engine(name) as e:
        e.set_excluded(x)
        _same(e.scan(q, 10), SR.answer(d, 10, excluded=x), (name, "excluded"))
        e.set_labels(lab)
        _same(e.scan(q, 10, a, b), SR.answer(d, 10, excluded=x, labels=lab, any_=a, all_=b), (name, "excluded, filters"))


@pytest.mark.parametrize("name", ["i8_100", "f32_1023"])
def test_a_packed_table_that_ends_its_buffer(name):
    """host placement on a caller's vector buffer of exactly N rows: no load may touch a byte behind the last row"""
    import bang_amd
    from bang_amd import binding as B
    ix, q = _get(name)
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)
    source = lambda first, count, dst: C.memmove(dst, graph[first:first + count].ctypes.data, count * ix.entry_len) and 0    # noqa: E731
    buf = B.DeviceBuffer(ix.N * ix.D * (4 if ix.dtype == "float" else 1))
    with bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_HOST, pull=1, distance=bang_amd.DISTANCE_EXACT, any_dim=1, scan_any=1) as e:
        e.load_stream(ix, source, d_vectors=buf.ptr)
        for k in (10, 128):
            _same(e.scan(q, k), SR.answer(_dist(name), k), (name, k))


def test_default_and_routing(small_u8, small_f32):
    import bang_amd
    for name, word in (("u8_100", "bang_search_can_rerank"), ("u8_48", "bang_search_can_rerank"), ("f32_96_mips", "MIPS search parameters are set")):
        with _engine(name, scan_any=0) as e:                   # without the option: today's codes and messages
            with pytest.raises(bang_amd.BangError, match=r"code -5.*" + word):
                e.scan(_get(name)[1], 10)
    for ix, q, _, _ in (small_u8, small_f32):                  # with it, a narrow layout returns what it returns without
        got = []
        for scan_any in (0, 1):
            with _engine("", ix, scan_any=scan_any) as e:
                got.append(e.scan(q, 100))
        _same(got[1], got[0], ix.dtype)
        _same(got[1], SR.answer(SR.distances(ix, q), 100), ix.dtype)


def _raw_refused(e, q, k, code, word):
    """bang_scan_e on caller-owned, sentinel-filled outputs"""
    from bang_amd import binding as B
    lib, Q = B.lib(), q.shape[0]
    lib.bang_scan_e.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ids, dists, matched = np.full((Q, k), 7, np.uint64), np.full((k, Q), 7.5, np.float32), np.full(Q, 7, np.uint32)
    rc = lib.bang_scan_e(e._h, q.ctypes.data, Q, k, None, None, ids.ctypes.data, dists.ctypes.data, matched.ctypes.data)
    msg = lib.bang_last_error().decode()
    assert rc == code and "bang_scan" in msg and word in msg, (rc, msg)
    assert (ids == 7).all() and (dists == 7.5).all() and (matched == 7).all(), ("a refused call wrote an output", word)


def test_refusals_with_the_option(small_f32):
    import bang_amd
    from bang_amd import binding as B
    ix, q = small_f32[:2]
    with _engine("", ix, graph=bang_amd.GRAPH_HOST, pull=1, vectors_fp16=1) as e:
        _raw_refused(e, q, 10, -5, "fp16")
    with _engine("u8_100") as e:
        _raw_refused(e, _get("u8_100")[1], 129, -1, "k = 129")
    lib = B.lib()                                              # the kernel entry: refused before any HIP call, the buffers as they were
    lib.bang_k_scan_any.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    for dtype, D, word in ((0, 18, "D % 4 == 0"), (2, 1028, "D = 1028")):
        Q, k, size = 8, 10, D * (4 if dtype == 2 else 1)
        bufs = [B.DeviceBuffer.from_numpy(np.full(n, 7, np.uint32)) for n in (64 * size, Q * size, 1024, 2 * Q * k, Q * k, Q)]
        p = B.ScanParams()
        p.d_vec_base, p.vec_stride, p.dtype, p.D, p.n_nodes, p.d_queries, p.nq, p.k = bufs[0].ptr, (size + 3) & ~3, dtype, D, 64, bufs[1].ptr, Q, k
        p.d_scratch, p.scratch_bytes, p.d_ids_out, p.d_dists_out, p.d_matched = bufs[2].ptr, 4096, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr
        assert lib.bang_k_scan_any(C.byref(p), D, None) == -5 and word in lib.bang_last_error().decode(), lib.bang_last_error().decode()
        assert all((b.download(np.uint32, (n,)) == 7).all() for b, n in zip(bufs[3:], (2 * Q * k, Q * k, Q))), (D, "a refused launch wrote an output")
        for b in bufs:
            b.free()
