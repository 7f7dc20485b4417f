"""Option any_dim of the exact-distance search mode (the any-dimension instances of csrc/bang_search_exact.hip) on the inputs of tests/anydim_inputs.py:
bit parity with the CPU reference on both placements, one wave on a packed table that ends its buffer, the default, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import anydim_inputs as A
from exact_reference import Reference

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]


def _engine(ix, placement="device", any_dim=1, **opts):
    import bang_amd
    opts.update(dict(graph=bang_amd.GRAPH_HOST, pull=1) if placement == "pulled" else dict(graph=bang_amd.GRAPH_DEVICE))
    return bang_amd.Engine(ix.dtype, distance=bang_amd.DISTANCE_EXACT, any_dim=any_dim, **opts)


def _check(e, name, q, k, L, want):                        # one run: ids, distance bits and the four per-query counters equal the reference's
    import bang_amd
    e.set_searchparams(k, L, bang_amd.DIST_MIPS if A.is_mips(name) else bang_amd.DIST_L2)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    st = e.query_counters(q.shape[0])
    e.free()
    assert np.array_equal(ids, want[0]) and np.array_equal(d.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(st, want[2])


@pytest.mark.parametrize("placement", ["device", "pulled"])
@pytest.mark.parametrize("name", A.NAMES)
def test_any_dimension_layouts_match_the_reference_bit_for_bit(name, placement):
    ix, q = A.get(name)
    with _engine(ix, placement) as e:
        e.load_index(ix)
        for k, L in A.KL:
            _check(e, name, q, k, L, A.reference(name, k, L))
            s = e.stats()
            assert s["search_kernel"] == 1 and s["rerank_fused"] == 0 and s["graph_pull"] == (1 if placement == "pulled" else 0), s


@pytest.mark.parametrize("name", ["i8_100", "f32_1023"])
def test_one_wave_on_a_packed_table_that_ends_its_buffer(name, monkeypatch):
    """The pulled form on a caller's vector buffer of exactly N rows (no load may touch a byte outside a row: there for the rule), one wave running every query."""
    from bang_amd import binding as B
    monkeypatch.setenv("BANG_SEARCH_MAX_WGS", "1")
    monkeypatch.setenv("BANG_SEARCH_MAX_WAVES", "1")
    ix, q = A.get(name)
    graph = np.ascontiguousarray(ix.graph, dtype=np.uint8)
    source = lambda first, count, dst: C.memmove(dst, graph[first:first + count].ctypes.data, count * ix.entry_len) and 0    # noqa: E731
    buf = B.DeviceBuffer(ix.N * ix.D * (4 if ix.dtype == "float" else 1))
    with _engine(ix, "pulled") as e:
        e.load_stream(ix, source, d_vectors=buf.ptr)
        _check(e, name, q, 10, 37, A.reference(name, 10, 37))


def test_default_is_what_it_was(small_u8):
    import bang_amd
    for name in ("u8_100", "f32_5", "f32_96_mips"):            # without the option: refused, with the messages of today
        ix, q = A.get(name)
        with _engine(ix, any_dim=0) as e:
            e.load_index(ix)
            with pytest.raises(bang_amd.BangError, match=r"no MIPS" if name == "f32_96_mips" else r"distance = 1 \(exact\): unsupported vector layout"):
                _check(e, name, q, 10, 37, None)
    ix8, q8, _, _ = small_u8                                   # with it, a layout of today's instances returns what it returns without
    want = Reference(ix8).search(q8, 10, 37, "exact")
    for any_dim in (0, 1):
        with _engine(ix8, any_dim=any_dim) as e:
            e.load_index(ix8)
            _check(e, "small_u8", q8, 10, 37, want)


@pytest.mark.parametrize("what", ["beam", "set_filters", "set_radii", "insert", "scan"])
def test_everything_but_the_plain_walk_is_refused_by_name(what):
    import bang_amd
    ix, q = A.get("u8_100")
    Q, ones = q.shape[0], np.ones(q.shape[0], np.uint32)
    call = {"beam": lambda e: e.alloc(Q), "insert": lambda e: e.insert(ix.vectors()[:4], 37), "scan": lambda e: e.scan(q, 10),
            "set_filters": lambda e: (e.alloc(Q), e.set_filters(ones, ones)), "set_radii": lambda e: (e.alloc(Q), e.set_radii(ones.astype(np.float32)))}
    with _engine(ix, **(dict(beam=2) if what == "beam" else {})) as e:
        e.load_index(ix)
        e.set_searchparams(10, 37)
        with pytest.raises(bang_amd.BangError, match=r"code -5.*any_dim = 1"):
            call[what](e)
