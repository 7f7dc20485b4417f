"""Re-use of removed ids on a GPU (csrc/bang_reuse.hip, bang_insert_reuse_e, bang_set_removed_e), byte for byte against tests/reuse_reference.py:
bang_k_bitmap_select against np.flatnonzero at the seams of a word, of a workgroup's span (32768 bits) and of the scan of the span counts (256
spans); bang_k_copy_rows_by_id in both directions on its three alignment paths and with rows 32 MiB apart; the engine on every case of
tests/reuse_inputs.py -- ids, entries, codes, the removed set, the counters --, under the chunk hooks, with an empty free set against bang_insert_e,
after its refusals; the exact scan and three search forms afterwards; a second consolidation; the removed set through its sidecar file into a
fresh engine; and the refusals of bang_set_removed_e.

Run time of the CPU references these tests wait for: see tests/test_reuse_reference.py."""
import ctypes as C

import numpy as np
import pytest

import consolidate_inputs as CI
import consolidate_reference as CR
import insert_inputs as I
import reuse_inputs as RI
import reuse_reference as RR
import scan_reference as SR
from exact_reference import Reference

pytestmark = pytest.mark.gpu

K, L = 10, 48
MARK = 0xCDCDCDCD
SPAN = 32768                                # BANG_SELECT_SPAN_BITS: the bits of one workgroup; 256 spans = one pass of the scan's threads


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _d2h(ptr, nbytes):
    from bang_amd import binding as B
    out = np.empty(nbytes, np.uint8)
    B._check(B.lib().bang_dev_d2h(B._vp(out), C.c_void_p(ptr), C.c_size_t(nbytes)), "bang_dev_d2h")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# bang_k_bitmap_select
# ---------------------------------------------------------------------------------------------------------------------
def _pattern(kind, n_bits, rng):
    bits = np.zeros(n_bits, bool)
    if kind == "full":
        bits[:] = True
    elif kind == "last":
        bits[-1] = True
    elif kind == "first":
        bits[0] = True
    elif kind == "half":
        bits = rng.random(n_bits) < 0.5
    elif kind == "sparse":
        bits = rng.random(n_bits) < 0.001
    else:
        assert kind == "empty"
    return bits


def _words(bits, tail):
    """the bitmap's words; `tail`: what the bits of the last word at or behind n_bits are set to"""
    n = len(bits)
    padded = np.full((n + 31) // 32 * 32, tail, bool)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32)


def _select(d_a, d_not, n_bits, want, scratch):
    """-> (ids [min(want, total)], total); asserts the guard words behind the ids"""
    from bang_amd import binding as B
    guard = 8
    out = B.DeviceBuffer.from_numpy(np.full(want + guard, MARK, np.uint32))
    tot = B.DeviceBuffer.from_numpy(np.full(2, MARK, np.uint32))
    fn = B.lib().bang_k_bitmap_select
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    B._check(fn(d_a, d_not, n_bits, want, out.ptr, tot.ptr, scratch.ptr, None), "bang_k_bitmap_select")
    B.sync()
    got, t = out.download(np.uint32, (want + guard,)), tot.download(np.uint32, (2,))
    out.free()
    tot.free()
    assert t[1] == MARK, "a word behind d_total was written"
    k = min(want, int(t[0]))
    assert (got[k:] == MARK).all(), "written behind d_ids_out[min(want, total)]"
    return got[:k], int(t[0])


SMALL = (1, 31, 32, 33, 2047, 2048, 2049, SPAN - 1, SPAN, SPAN + 1)
LARGE = ((1 << 22) + 1, 256 * SPAN - 1, 256 * SPAN, 256 * SPAN + 1)     # 129 spans; one below, at and above one span per thread of the scan


@pytest.mark.parametrize("n_bits", SMALL + LARGE)
def test_bitmap_select_against_flatnonzero(n_bits):
    from bang_amd import binding as B
    B.lib().bang_bitmap_select_scratch_words.restype = C.c_uint64
    B.lib().bang_bitmap_select_scratch_words.argtypes = [C.c_uint32]
    rng = np.random.default_rng(n_bits)
    scratch = B.DeviceBuffer(4 * int(B.lib().bang_bitmap_select_scratch_words(n_bits)) + 16)
    kinds = ("empty", "full", "last", "first", "half", "sparse") if n_bits in SMALL else ("last", "half", "sparse")
    for kind in kinds:
        a = _pattern(kind, n_bits, rng)
        nt = rng.random(n_bits) < 0.3
        nt[-1] = False                                                    # (the last bit stays selectable)
        d_a = B.DeviceBuffer.from_numpy(_words(a, True))                  # the bits behind n_bits: set in a, clear in not -- selected unless masked
        d_not = B.DeviceBuffer.from_numpy(_words(nt, False))
        for with_not in (False, True):
            want_ids = np.flatnonzero(a & ~nt if with_not else a).astype(np.uint32)
            total = len(want_ids)
            wants = sorted({0, 1, max(total - 1, 0), total, total + 5, 16384}) if n_bits in SMALL else sorted({0, total, 16384})
            for want in wants:
                if want > (1 << 20):
                    want = 1 << 20                                        # (an output of 2^22 ids shows nothing more)
                ids, t = _select(d_a.ptr, d_not.ptr if with_not else None, n_bits, want, scratch)
                assert t == total, (kind, with_not, want)
                assert np.array_equal(ids, want_ids[:want]), (kind, with_not, want)
        d_a.free()
        d_not.free()
    scratch.free()


# ---------------------------------------------------------------------------------------------------------------------
# bang_k_copy_rows_by_id
# ---------------------------------------------------------------------------------------------------------------------
def _copy(table_ptr, table_stride, byte_offset, ids, n_nodes, packed_ptr, packed_stride, nbytes, to_table):
    """-> abort word"""
    from bang_amd import binding as B
    d_ids = B.DeviceBuffer.from_numpy(np.asarray(ids, np.uint32))
    ab = B.DeviceBuffer(4)
    fn = B.lib().bang_k_copy_rows_by_id
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    B._check(fn(table_ptr, table_stride, byte_offset, d_ids.ptr, len(ids), n_nodes, packed_ptr, packed_stride, nbytes, int(to_table), ab.ptr, None),
             "bang_k_copy_rows_by_id")
    B.sync()
    abort = int(ab.download(np.uint32, (1,))[0])
    d_ids.free()
    ab.free()
    return abort


# (table stride, byte offset, bytes, packed stride): the byte path (a stride of 70; an odd offset), the dword path (196-byte entries: a whole
# entry, its row behind a 64-byte vector, one word), the 16-byte path (128-byte rows; 640-byte rows whose 532 bytes end in a dword)
COPY_SHAPES = [(70, 0, 70, 70), (70, 3, 4, 5), (70, 0, 70, 72), (196, 0, 196, 196), (196, 64, 132, 132), (196, 64, 4, 8), (198, 1, 132, 133),
               (128, 0, 128, 128), (128, 16, 70, 80), (128, 0, 4, 16), (640, 0, 516 + 16, 544), (640, 64, 196, 208), (640, 128, 132, 144)]
COPY_NODES = 300


@pytest.mark.parametrize("shape", COPY_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_copy_rows_by_id_both_directions(shape):
    from bang_amd import binding as B
    ts, off, nb, ps = shape
    rng = np.random.default_rng(sum(shape))
    table = rng.integers(0, 256, (COPY_NODES, ts), dtype=np.uint8)
    d_table = B.DeviceBuffer.from_numpy(table, slack=256)
    # table -> packed: unsorted ids, some twice, one outside the table (skipped, reported); 9 rows: three workgroups, the last one wave
    ids = np.concatenate([rng.choice(COPY_NODES, 6, replace=False), [COPY_NODES + 7]]).astype(np.uint32)
    ids = np.concatenate([ids, ids[[2, 0]]]).astype(np.uint32)
    n = len(ids)
    packed = np.full((n, ps), 0xA5, np.uint8)
    d_packed = B.DeviceBuffer.from_numpy(packed, slack=64)
    assert _copy(d_table.ptr, ts, off, ids, COPY_NODES, d_packed.ptr, ps, nb, False) == 2, "the id outside the table was not reported"
    got = d_packed.download(np.uint8, (n, ps))
    want = packed.copy()
    for i, x in enumerate(ids):
        if x < COPY_NODES:
            want[i, :nb] = table[x, off:off + nb]
    assert np.array_equal(got, want), "the rows, and no byte between them"
    assert np.array_equal(d_table.download(np.uint8, table.shape), table), "the read side was written"
    # packed -> table: distinct ids (and the outsider); every other byte of the table stays
    wids = np.concatenate([rng.choice(COPY_NODES, 8, replace=False), [COPY_NODES]]).astype(np.uint32)
    src = rng.integers(0, 256, (len(wids), ps), dtype=np.uint8)
    d_packed.upload(src)
    assert _copy(d_table.ptr, ts, off, wids, COPY_NODES, d_packed.ptr, ps, nb, True) == 2
    want = table.copy()
    for i, x in enumerate(wids[:-1]):
        want[x, off:off + nb] = src[i, :nb]
    assert np.array_equal(d_table.download(np.uint8, table.shape), want), "the rows, and no byte between them"
    assert np.array_equal(_d2h(d_table.ptr + table.nbytes, 256), np.zeros(256, np.uint8)), "written behind the table"
    # all ids inside: the abort word stays 0
    assert _copy(d_table.ptr, ts, off, wids[:-1], COPY_NODES, d_packed.ptr, ps, nb, True) == 0
    d_table.free()
    d_packed.free()


@pytest.mark.parametrize("row", [196, 128, 70])
def test_copy_row_addressing_beyond_4_gib(row):
    """table rows 32 MiB (+ the row) apart, ids >= 160: id * table_stride passes 4 GiB (5 GiB at id 160); the three alignment paths.  A kernel that
    wrapped the offset at 32 bits would read / write row (id * stride) mod 2^32 -- inside the buffer, where the marks and zeros are checked"""
    import stretch_inputs as S
    from bang_amd import binding as B
    stride = S.stride_of(row)
    NN = 170
    assert 160 * stride > (4 << 30)
    rng = np.random.default_rng(row)
    buf = S.device_buffer(NN * stride + 256)
    ids = np.array([165, 160, 3, 169, 161], np.uint32)
    rows = rng.integers(1, 256, (len(ids), row), dtype=np.uint8)
    for i, x in enumerate(ids):
        buf.upload(rows[i], int(x) * stride)
    ps = (row + 15) // 16 * 16 if row % 16 == 0 else row
    d_packed = B.DeviceBuffer.from_numpy(np.full((len(ids), ps), 0xA5, np.uint8), slack=64)
    assert _copy(buf.ptr, stride, 0, ids, NN, d_packed.ptr, ps, row, False) == 0
    assert np.array_equal(d_packed.download(np.uint8, (len(ids), ps))[:, :row], rows), "the far rows came back"
    # ... and the other way, to other far rows
    wids = np.array([168, 2, 162, 167], np.uint32)
    src = rng.integers(1, 256, (len(wids), ps), dtype=np.uint8)
    d_packed.upload(src)
    assert _copy(buf.ptr, stride, 0, wids, NN, d_packed.ptr, ps, row, True) == 0
    for i, x in enumerate(wids):
        at = int(x) * stride
        got = _d2h(buf.ptr + at - 64, row + 128) if x else _d2h(buf.ptr, row + 64)
        lead = 64 if x else 0
        assert np.array_equal(got[lead:lead + row], src[i, :row]), (x, "the row")
        assert not got[:lead].any() and not got[lead + row:].any(), (x, "bytes around the row")
        wrapped = at % (1 << 32)
        if wrapped != at:
            assert not _d2h(buf.ptr + wrapped, row).any() or wrapped // stride in ids, (x, "the row landed at its offset modulo 2^32")
    buf.free()
    d_packed.free()


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def _engine(ix, capacity, **opts):
    import bang_amd
    e = bang_amd.Engine(ix.dtype, graph=bang_amd.GRAPH_DEVICE, **(dict(capacity=capacity) if capacity is not None else {}), **opts)
    e.load_index(ix)
    return e


def _prepare(e, run):
    """the run's consolidation and its exclusion set, on an engine loaded with run.ix0"""
    e.set_excluded(run.x)
    st = e.consolidate(run.alpha_c)
    assert st["removed"] == len(run.removed)
    e.set_excluded(run.excluded)
    assert np.array_equal(e.entries(0, run.ix1.N), run.ix1.graph)
    assert np.array_equal(e.removed_ids(), run.removed)
    assert e.free_slots() == dict(free=len(run.removed), eligible=len(RR.eligible(run.removed, run.excluded)), reused=0)


def _check_step(e, run, s, reused):
    assert e.num_nodes() == s.ix.N
    assert np.array_equal(e.entries(0, s.ix.N), s.ix.graph), "graph entries"
    assert np.array_equal(e.codes(0, s.ix.N), s.ix.codes), "code rows"
    assert np.array_equal(e.removed_ids(), s.removed), "the removed set"
    assert e.free_slots() == dict(free=len(s.removed), eligible=len(RR.eligible(s.removed, run.excluded)), reused=reused)


def _run_steps(e, run):
    reused = 0
    for s in run.steps:
        ids = e.insert_reuse(s.vectors, run.L, run.alpha)
        assert ids.dtype == np.uint64 and np.array_equal(ids, s.ids.astype(np.uint64)), "the ids of the batch"
        reused += s.stats["reused"]
        _check_step(e, run, s, reused)
        st = e.insert_stats()
        t = e.insert_times()
        assert t["total"] > 0 and t["search"] > 0 and t["group"] > 0
    return st


@pytest.mark.parametrize("name", sorted(RI.CASES))
def test_insert_reuse_matches_the_reference_byte_for_byte(name):
    from bang_amd import BangError
    run = RI.reference(name)
    with _engine(run.ix0, run.capacity) as e:
        _prepare(e, run)
        if name == "exact_fit":
            with pytest.raises(BangError, match="bang_insert:.*capacity"):
                e.insert(run.steps[0].vectors, run.L, run.alpha)           # capacity == N: the appending insert has no room
        st = _run_steps(e, run)
        assert st["inserted"] == sum(len(s.ids) for s in run.steps)
        assert st["backedge_appended"] == sum(s.stats["appended"] for s in run.steps)
        assert st["backedge_pruned"] == sum(s.stats["pruned"] for s in run.steps)


@pytest.mark.parametrize("name,chunks", [("mixed", (20, 64, 7)), ("u8", (33, 100, 50)), ("deep", (1, 1, 1)), ("all_free", (5, 3, 16))])
def test_the_chunk_hooks_change_nothing(name, chunks, monkeypatch):
    run = RI.reference(name)
    for key, val in zip(("BANG_INSERT_SEARCH_CHUNK", "BANG_INSERT_TARGET_CHUNK", "BANG_INSERT_ENCODE_CHUNK"), chunks):
        monkeypatch.setenv(key, str(val))
    with _engine(run.ix0, run.capacity) as e:
        _prepare(e, run)
        _run_steps(e, run)


@pytest.mark.parametrize("name", ["i8_a12", "u8_a12"])
def test_an_empty_free_set_gives_the_bytes_of_the_plain_insert(name):
    ix, v, Lb, alpha = I.case(name)
    ix2, _ = I.reference(name)
    with _engine(ix, ix.N + len(v)) as a, _engine(ix, ix.N + len(v)) as b:
        assert a.insert(v, Lb, alpha) == ix.N
        ids = b.insert_reuse(v, Lb, alpha)
        assert np.array_equal(ids, ix.N + np.arange(len(v), dtype=np.uint64))
        assert a.num_nodes() == b.num_nodes() == ix2.N
        ea, eb = a.entries(0, ix2.N), b.entries(0, ix2.N)
        assert np.array_equal(ea, eb) and np.array_equal(a.codes(0, ix2.N), b.codes(0, ix2.N)), "two engines, one result"
        assert np.array_equal(eb, ix2.graph) and np.array_equal(b.codes(0, ix2.N), ix2.codes)
        assert a.insert_stats() == b.insert_stats() and b.free_slots() == dict(free=0, eligible=0, reused=0) and b.removed_ids().size == 0


def _exact_ids(e, q):
    e.set_option("distance", 1)
    e.set_option("search", 1)
    e.set_searchparams(K, L)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    e.free()
    return ids, _bits(d)


def test_refusals_leave_no_trace():
    import bang_amd
    from bang_amd import BangError, binding as B
    run = RI.reference("mixed")
    s = run.steps[0]
    q = np.ascontiguousarray(I.get("i8")[1][:8])
    N = run.ix1.N
    with _engine(run.ix0, N + 10) as e:                                    # the batch needs N + 24
        _prepare(e, run)
        before = _exact_ids(e, q)                                          # (walks from the seed list)

        def refused(match, v=s.vectors, Lb=run.L, a=run.alpha):
            with pytest.raises(BangError, match="bang_insert_reuse.*" + match):
                e.insert_reuse(v, Lb, a)
        refused("capacity")
        refused("n = 0", v=s.vectors[:0])
        refused("alpha", a=0.5)
        refused("alpha", a=float("nan"))
        refused("L_build", Lb=0)
        e.set_labels(np.ones(N, np.uint32))
        refused("label")
        e.clear_labels()
        e.set_searchparams(K, 40)
        e.alloc(8)
        refused("allocation")
        e.free()
        e.set_searchparams(K, 40, bang_amd.DIST_MIPS)
        refused("MIPS")
        e.set_searchparams(K, 40)
        fn = B.lib().bang_insert_reuse_e
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
        assert fn(e._h, B._vp(s.vectors), 16, run.L, C.c_float(run.alpha), None) == -1
        assert "ids_out" in B.lib().bang_last_error().decode()
        assert e.num_nodes() == N and np.array_equal(e.entries(0, N), run.ix1.graph) and np.array_equal(e.codes(0, N), run.ix1.codes)
        assert np.array_equal(e.removed_ids(), run.removed) and e.free_slots()["reused"] == 0 and e.insert_stats()["inserted"] == 0
        after = _exact_ids(e, q)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the seed list moved"
        # ... and the engine still inserts: the 24 points that fit the free slots
        ids = e.insert_reuse(s.vectors[:24], run.L, run.alpha)
        assert np.array_equal(ids, run.removed.astype(np.uint64)) and e.num_nodes() == N
    with _engine(run.ix0, None) as e:                                      # no capacity
        with pytest.raises(BangError, match="bang_insert_reuse.*capacity"):
            e.insert_reuse(s.vectors, run.L, run.alpha)


# ---------------------------------------------------------------------------------------------------------------------
# afterwards
# ---------------------------------------------------------------------------------------------------------------------
FORMS = {"exact": dict(distance=1, search=1, beam=1), "pq": dict(distance=0, search=1, beam=1), "beam2": dict(distance=1, search=1, beam=2)}


def _search(e, q, form):
    for key, val in FORMS[form].items():
        e.set_option(key, val)
    e.set_searchparams(K, L)
    e.alloc(q.shape[0])
    e.init(q.shape[0])
    ids, d = e.query(q)
    out = (ids, _bits(d), e.query_counters(q.shape[0]))
    e.free()
    return out


def _form_reference(ix2, q, form):
    if form == "exact":
        ids, d, st = Reference(ix2).search(q, K, L, "exact")
    elif form == "beam2":
        import beam_reference
        ids, d, st = beam_reference.Reference(ix2).search(q, K, L, 2)[:3]
    else:
        from oracle import oracle as O
        ids, d, st = O.Oracle(ix2).search(q, K, L, with_stats=True)
    return ids, _bits(d), st


def test_scan_and_searches_after_a_reuse():
    """case "mixed" (F and X end empty): the scan finds every new point at its id and distance 0; the exact walk, the PQ walk and the beam form
    answer 24 queries -- 16 of the index's, 8 of the new vectors -- as their CPU references do on the reference's Index'; then a second
    consolidation that deletes six re-used slots, two appended ids and eight nodes around node 700 matches consolidate_reference"""
    run = RI.reference("mixed")
    s = run.steps[0]
    ix2 = s.ix
    q = np.ascontiguousarray(np.concatenate([I.get("i8")[1][:16], s.vectors[:8]]))
    with _engine(run.ix0, run.capacity) as e:
        _prepare(e, run)
        _run_steps(e, run)
        got = e.scan(s.vectors, 4)
        want = SR.answer(SR.distances(ix2, s.vectors), 4, removed=s.removed)
        assert SR.same(got, want), SR.first_difference(got, want)
        assert (_bits(got[1][0]) == 0).all(), "a new point is not at distance 0 of its own vector"
        for i, x in enumerate(s.ids):
            zero = got[0][i][_bits(got[1][:, i]) == 0]
            assert int(x) in zero and list(zero) == sorted(zero), (i, "its id among the zero distances, ties in id order")
        assert (got[0][:, 0] != s.ids).any(), "no new point ties with an older copy: the tie rule was not exercised"
        for form in FORMS:
            mine = _search(e, q, form)
            for a, b, part in zip(mine, _form_reference(ix2, q, form), ("ids", "distance bits", "counters")):
                assert np.array_equal(a, b), (form, part)
            assert np.isin(mine[0][16:], s.ids.astype(np.uint64)).any(), (form, "no query finds a new point")
        x2 = np.concatenate([s.ids[:6], s.ids[-2:], CI.ball(ix2, 700, 8)]).astype(np.uint32)
        ix3, st3, remaining = CR.consolidate(ix2, x2, 1.2)
        assert len(remaining) == 0 and (s.ids[:6] < run.ix1.N).all() and (s.ids[-2:] >= run.ix1.N).all()
        e.set_excluded(x2)
        assert e.consolidate(1.2)["removed"] == st3["removed"]
        assert np.array_equal(e.entries(0, ix3.N), ix3.graph)
        in_d, _ = CR.split(ix2, x2)
        assert np.array_equal(e.removed_ids(), np.flatnonzero(in_d)), "the re-used slots are free again"


def test_scan_never_returns_a_free_slot():
    """case "excluded_again": three slots stay free (and excluded), one live node is excluded; the vectors of all four as queries"""
    run = RI.reference("excluded_again")
    s = run.steps[0]
    qs = np.ascontiguousarray(np.concatenate([run.ix0.vectors()[run.excluded], s.vectors[:4]]))
    with _engine(run.ix0, run.capacity) as e:
        _prepare(e, run)
        _run_steps(e, run)
        got = e.scan(qs, K)
        want = SR.answer(SR.distances(s.ix, qs), K, excluded=run.excluded, removed=s.removed)
        assert SR.same(got, want), SR.first_difference(got, want)
        assert len(s.removed) == 3 and not np.isin(got[0], s.removed.astype(np.uint64)).any(), "a slot still in F was returned"
        assert not np.isin(got[0], run.excluded.astype(np.uint64)).any()
        assert np.isin(got[0], s.ids.astype(np.uint64)).any(), "the re-used slots are scanned again"


def test_the_removed_set_survives_an_export(tmp_path):
    """case "all_free" behind its first batch (14 slots still free): export, the sidecar, a fresh engine, set_removed -- then both engines scan
    alike and take the second batch at the same ids with the same bytes"""
    from bang_amd import formats
    run = RI.reference("all_free")
    s1, s2 = run.steps
    qs = np.ascontiguousarray(np.concatenate([run.ix0.vectors()[s1.removed[:6]], s1.vectors[:4]]))
    prefix = str(tmp_path / "ix")
    with _engine(run.ix0, run.capacity) as e:
        _prepare(e, run)
        assert np.array_equal(e.insert_reuse(s1.vectors, run.L, run.alpha), s1.ids.astype(np.uint64))
        exported = e.export_index(run.ix0)
        formats.write_index(prefix, exported)
        formats.write_removed(prefix, e.removed_ids())
        mine = e.scan(qs, K)
        loaded = formats.read_index(prefix, run.ix0.dtype)
        assert np.array_equal(loaded.graph, s1.ix.graph) and np.array_equal(formats.read_removed(prefix), s1.removed)
        with _engine(loaded, run.capacity) as f:
            naive = f.scan(qs, K)
            assert np.isin(naive[0], s1.removed.astype(np.uint64)).any(), "without the sidecar the removed nodes are scanned: the test would show nothing"
            f.set_removed(formats.read_removed(prefix))
            assert np.array_equal(f.removed_ids(), s1.removed) and f.free_slots() == dict(free=14, eligible=14, reused=0)
            theirs = f.scan(qs, K)
            assert SR.same(theirs, mine), SR.first_difference(theirs, mine)
            assert not np.isin(theirs[0], s1.removed.astype(np.uint64)).any()
            for eng in (e, f):
                assert np.array_equal(eng.insert_reuse(s2.vectors, run.L, run.alpha), s2.ids.astype(np.uint64))
                assert np.array_equal(eng.entries(0, s2.ix.N), s2.ix.graph) and np.array_equal(eng.codes(0, s2.ix.N), s2.ix.codes)
                assert eng.removed_ids().size == 0 and eng.num_nodes() == s2.ix.N
            f.set_removed([])                                              # n = 0 clears an empty set too
            assert f.removed_ids().size == 0


def test_set_removed_refusals_keep_the_old_set():
    from bang_amd import BangError
    run = RI.reference("mixed")
    ix1, N, med = run.ix1, run.ix1.N, int(run.ix1.medoid)
    listed = ix1.adjacency()[np.arange(ix1.R)[None, :] < ix1.degrees()[:, None]]
    live = int(np.setdiff1d(np.unique(listed), [med])[5])                  # a live node: its row is not empty, and rows list it
    with _engine(ix1, N) as e:                                             # the consolidated index, loaded afresh: F is empty
        assert e.removed_ids().size == 0
        e.set_removed(run.removed[::-1])                                   # (any order, duplicates are fine)
        assert np.array_equal(e.removed_ids(), run.removed)
        keep = run.removed[:5]
        e.set_removed(np.concatenate([keep, keep]))
        assert np.array_equal(e.removed_ids(), keep)
        for bad, match in (([N], f"id {N} .*out of range"), ([med], "medoid"), ([live], f"id {live} .*not empty")):
            with pytest.raises(BangError, match="bang_set_removed.*" + match):
                e.set_removed(np.concatenate([run.removed[5:9], bad]))
            assert np.array_equal(e.removed_ids(), keep), "a refused call replaced the set"
        e.set_searchparams(K, L)
        e.alloc(4)
        with pytest.raises(BangError, match="bang_set_removed.*allocation"):
            e.set_removed(run.removed)
        e.free()
        assert np.array_equal(e.removed_ids(), keep)
        e.set_removed([])
        assert e.removed_ids().size == 0 and e.free_slots() == dict(free=0, eligible=0, reused=0)
    # a node whose row is empty but that a live row still lists
    emptied = CI.with_rows(ix1, {live: []})
    owners = np.flatnonzero((emptied.adjacency() == live).any(axis=1) & (emptied.degrees() > 0))
    owners = [int(p) for p in owners if live in emptied.adjacency()[p, :emptied.degrees()[p]]]
    assert owners
    with _engine(emptied, N) as e:
        e.set_removed(run.removed[:3])
        with pytest.raises(BangError, match=f"bang_set_removed.*row of node {owners[0]},.*names a listed id"):
            e.set_removed([live])
        assert np.array_equal(e.removed_ids(), run.removed[:3])
    with _engine(ix1, None) as e:                                          # graph = device without capacity: the set may still be restored (for the scan)
        e.set_removed(run.removed)
        assert np.array_equal(e.removed_ids(), run.removed)
