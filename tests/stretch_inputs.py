"""Tables laid out at STRETCHED strides: a few hundred rows 32 MiB apart reach the byte offsets beyond 4 GiB (and beyond 16 GiB, where an
offset counted in dwords leaves 32 bits) that 10^8 nodes 128 bytes apart reach -- in milliseconds, at the kernel-level entries, which all take
their strides as arguments.  The stride does not enter the semantics: the expected answer is the CPU reference on the compact index.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  tests/test_stretch_inputs.py asserts ON THE CPU REFERENCES that every case below
reads rows beyond both marks and that a kernel which wrapped an offset at 2^32 or 2^34 could not give the reference's answer;
tests/test_gpu_offsets64.py launches the cases.  Both take their parameters from CASES.

    INPUTS, get()      synth.make_index at N = 640, R = 32, Q = 16, one per layout a kernel distinguishes (the entries of
                       instance_inputs.ENTRIES have 8 to 12 queries and mostly R = 64, so none is taken over)
    stride_of()        32 MiB + the compact stride: the same residue mod 16 (aligned / unaligned code rows and the `& 3` tests take the branch they
                       take today); ids >= 128 lie beyond 4 GiB, ids >= 512 beyond 16 GiB
    stretched()        a table on the device at such a stride behind a zeroed lead-in of 2 GiB (an offset sign-extended from 32 bits still lands in
                       memory the test owns: wrong bits, not a fault) -- in a buffer of its own or in one it shares with another table
    wrapped()          the compact index a kernel would see if it wrapped the offsets of one table at 2^bits (plain numpy)
    walk()             the reference walk of a mode with what it read: code rows, vectors, graph entries, and the candidate logs
    reference()        the mode's own reference on an index as given
    CASES              (entry, input, mode, tables stretched, options) of every GPU case; cpu_params() = the (input, table, mode) they need
"""
from __future__ import annotations

import collections
import dataclasses
import functools

import numpy as np

from bang_amd import synth

GIB = 1 << 30
LEAD = 2 * GIB
BLOW = 32 << 20
SHARE_GAP = 16 << 20                  # two tables in one buffer: the second starts this far behind the first (rows never meet: N * row << 16 MiB)
N, R, Q, K, L = 640, 32, 16, 10, 37
WRAPS = (32, 34)

# name -> (D, dtype, m)
INPUTS = {
    "u8_128_m70": (128, "uint8", 70),     # code rows not dword-aligned: the ragged instance
    "u8_128_m32": (128, "uint8", 32),     # the aligned instance
    "i8_64_m16":  (64,  "int8",  16),
    "f32_128_m32": (128, "float", 32),
    "f32_96_m74": (96,  "float", 74),
    "u8_48":      (48,  "uint8", 12),     # wide, D / 16 = 3
    "f32_320":    (320, "float", 40),     # wide float, LDS tile
    "u8_130_m13": (130, "uint8", 13),     # LUT path (10-dimension chunks), rows unaligned
    "f32_100":    (100, "float", 25),     # fp16 re-rank only
    "f32_260":    (260, "float", 65),
}


@functools.lru_cache(maxsize=None)
def get(name: str):
    """-> (Index, queries [Q][D]); treat both as read-only."""
    D, dtype, m = INPUTS[name]
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=K, n_clusters=8, seed=5000 + D + m, device="cpu", pq_iters=2)
    return ix, np.ascontiguousarray(q)


def tsize(ix) -> int:
    return 4 if ix.dtype == "float" else 1


def stride_of(compact: int) -> int:
    return BLOW + int(compact)


def compact_stride(name: str, which: str, fp16: bool = False, vectors_in_graph: bool = False) -> int:
    """Bytes between two rows of a table of the input as the engine lays it out (needs no index)."""
    D, dtype, m = INPUTS[name]
    vb = D * (4 if dtype == "float" else 1)
    if which == "codes":
        return m
    if which == "graph" or vectors_in_graph:
        return vb + 4 + 4 * R
    return (2 * D + 3) & ~3 if fp16 else vb


# ------------------------------------------------------------------------------------------------------------------------ device side
def _rows(table: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(table)
    return t.reshape(t.shape[0], -1).view(np.uint8)


def device_buffer(nbytes: int):
    """A zeroed device buffer; a failed allocation FAILS the test and says so."""
    import pytest
    from bang_amd import binding as B
    try:
        return B.DeviceBuffer(nbytes)
    except B.BangError as e:
        pytest.fail(f"box too small for this test: {nbytes / GIB:.1f} GiB of device memory could not be allocated ({e})")


def stretched(table: np.ndarray, stride: int, lead: int = LEAD, into=None, at: int = 0):
    """-> (DeviceBuffer, device address of row 0).  A buffer of lead + N * stride + 256 zeroed bytes with row i at lead + i * stride; or,
    into = a buffer made earlier, row i at byte `at` + i * stride of that one."""
    from bang_amd import binding as B
    t = _rows(table)
    assert stride >= t.shape[1]
    buf = into if into is not None else device_buffer(lead + t.shape[0] * stride + 256)
    base = at if into is not None else lead
    assert base + (t.shape[0] - 1) * stride + t.shape[1] <= buf.nbytes
    B.upload_rows(buf, t, base, stride)
    return buf, buf.ptr + base


def stretched_pair(first: np.ndarray, stride1: int, second: np.ndarray, stride2: int):
    """Two tables at stretched strides in ONE buffer (two of 22 GiB would not fit the 24 GiB a test may hold): -> (buffer, address of
    `first`, address of `second`).  `first` starts behind the lead-in, `second` SHARE_GAP behind it; the rows of both drift by less than that."""
    a, b = _rows(first), _rows(second)
    rows = max(a.shape[0], b.shape[0])
    assert rows * (a.shape[1] + b.shape[1] + abs(stride1 - stride2)) < SHARE_GAP       # the drift between the two never closes the gap
    buf = device_buffer(LEAD + SHARE_GAP + max(a.shape[0] * stride1, b.shape[0] * stride2) + 256)
    _, p1 = stretched(a, stride1, into=buf, at=LEAD)
    _, p2 = stretched(b, stride2, into=buf, at=LEAD + SHARE_GAP)
    return buf, p1, p2


# ------------------------------------------------------------------------------------------------------------------------ what a wrap would read
def wrapped_table(table: np.ndarray, stride: int, bits: int) -> np.ndarray:
    """uint8 [N][row]: row i = the bytes at (i * stride) mod 2^bits of the stretched image -- zeros where no row lies, a shifted piece of
    another row where one does."""
    t = _rows(table)
    n, row = t.shape
    pos = (np.arange(n, dtype=np.int64)[:, None] * stride) % (1 << bits) + np.arange(row, dtype=np.int64)[None, :]
    j, w = pos // stride, pos % stride
    ok = (j < n) & (w < row)
    out = np.zeros_like(t)
    out[ok] = t[j[ok], w[ok]]
    return out


def wrapped(ix, which: str, stride: int, bits: int, fp16: bool = False):
    """The compact index a kernel would see if it wrapped the byte offsets of table `which` at 2^bits: "graph" (whole graph entries),
    "vectors" (the vector table, or the vector part of the entries where the kernel reads them there; fp16: the table holds halves) or
    "codes"."""
    if which == "codes":
        return dataclasses.replace(ix, codes=wrapped_table(ix.codes, stride, bits))
    if which == "graph":
        return dataclasses.replace(ix, graph=wrapped_table(ix.graph, stride, bits))
    assert which == "vectors"
    g = ix.graph.copy()
    vb = ix.D * tsize(ix)
    if fp16:
        h = wrapped_table(ix.vectors().astype(np.float16), stride, bits)
        g[:, :vb] = np.ascontiguousarray(h.view(np.float16).astype(np.float32)).view(np.uint8).reshape(ix.N, vb)
    elif stride - BLOW == ix.entry_len:                 # the vectors are read from the graph entries
        g[:, :vb] = wrapped_table(ix.graph, stride, bits)[:, :vb]
    else:
        g[:, :vb] = wrapped_table(ix.graph[:, :vb], stride, bits)
    return dataclasses.replace(ix, graph=g)


# ------------------------------------------------------------------------------------------------------------------------ references
MODES = ("base", "exact", "beam2", "beam4", "inmem", "wf", "fp16_base", "fp16_exact")


def _index_of(ix, mode: str):
    if mode.startswith("fp16"):
        import fp16_inputs
        return fp16_inputs.rounded(ix)
    return ix


def reference(ix, q, mode: str):
    """The mode's own reference at k = K, L = L on ix AS GIVEN (fp16 modes: on its rounded copy): (ids [Q][k], dists [k][Q], stats [Q][4], ...)"""
    ix = _index_of(ix, mode)
    if mode in ("base", "fp16_base"):
        from oracle import oracle as O
        return O.Oracle(ix).search(q, K, L, with_stats=True)
    if mode in ("exact", "fp16_exact"):
        from exact_reference import Reference
        return Reference(ix).search(q, K, L, "exact")
    if mode in ("beam2", "beam4"):
        from beam_reference import Reference
        return Reference(ix).search(q, K, L, int(mode[4]))[:3]
    if mode == "inmem":
        from inmemory_reference import Reference
        return Reference(ix).search(q, K, L, "inmemory")
    if mode == "wf":
        from wordfilter_reference import Reference
        return Reference(ix).search(q, K, L, "word")
    raise ValueError(mode)


def differs(a, b) -> bool:
    """ids or distance bits of at least one query"""
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


Walk = collections.namedtuple("Walk", "ids dists stats logs codes vectors graph")


class _Recorder:
    """Notes which rows a Reference object reads: adjacency() = graph entries, exact() / orc.exact_dist() = vectors, orc.pqdist() = code rows."""

    def __init__(self, ref):
        self.graph, self.vectors, self.codes = [], [], []
        adjacency, pqdist, exact_dist = ref.adjacency, ref.orc.pqdist, ref.orc.exact_dist
        ref.adjacency = lambda node: (self.graph.append(int(node)), adjacency(node))[1]
        ref.orc.pqdist = lambda lut, ids: (self.codes.extend(int(x) for x in ids), pqdist(lut, ids))[1]
        ref.orc.exact_dist = lambda node, *a: (self.vectors.append(int(node)), exact_dist(node, *a))[1]
        if hasattr(ref, "exact"):
            exact = ref.exact
            ref.exact = lambda ids, *a: (self.vectors.extend(int(x) for x in ids), exact(ids, *a))[1]


@functools.lru_cache(maxsize=None)
def walk(name: str, mode: str) -> Walk:
    """The reference walk of `mode` over the input's queries, query by query, with the candidate logs (one array per query) and the ids of the
    code rows, vectors and graph entries it read.  base: the walk of wordfilter_reference's split layout, which is Oracle.search's (asserted
    in tests/test_stretch_inputs.py) and also hands out its log."""
    ix, q = get(name)
    ix = _index_of(ix, mode)
    if mode in ("base", "fp16_base", "wf"):
        from wordfilter_reference import Reference
        ref = Reference(ix)
        layout = "word" if mode == "wf" else "split"

        def one(v):
            log = []
            return ref.search_one(v, K, L, layout, log=log) + (np.array(log, np.uint32),)
    elif mode in ("exact", "fp16_exact"):
        from exact_reference import Reference
        ref = Reference(ix)

        def one(v):
            n = len(rec.graph)
            out = ref.search_one(v, K, L, "exact")
            log = np.array(rec.graph[n:], np.uint32)           # every logged parent is expanded, unless the walk ends at the cap
            assert out[2][0] < L + 49 and len(log) == out[2][1], "the walk reached the iteration cap: choose another input"
            return out + (log,)
    elif mode in ("beam2", "beam4"):
        from beam_reference import Reference
        ref = Reference(ix)
        one = lambda v: ref.search_one(v, K, L, int(mode[4]))       # noqa: E731
    elif mode == "inmem":
        from inmemory_reference import Reference
        ref = Reference(ix)
        one = lambda v: ref.search_one_logged(v, K, L, "inmemory")  # noqa: E731
    else:
        raise ValueError(mode)
    rec = _Recorder(ref)
    ids, dists, st, logs = np.empty((Q, K), np.uint64), np.empty((K, Q), np.float32), np.empty((Q, 4), np.int64), []
    for i in range(Q):
        ids[i], dists[:, i], st[i], log = one(q[i])
        logs.append(np.asarray(log, np.uint32))
    u = lambda a: np.array(a, np.int64)                              # noqa: E731
    return Walk(ids, dists, st, logs, u(rec.codes), u(rec.vectors), u(rec.graph))


# ------------------------------------------------------------------------------------------------------------------------ the cases
# tables: which of "graph", "codes", "vectors" lie at a stretched stride.  opt: layout (row_layout), beam, f16, lut (use_lut), engine options.
Case = collections.namedtuple("Case", "entry input mode tables opt", defaults=((),))


def _opt(**kw):
    return tuple(sorted(kw.items()))


def _cases():
    out = []
    for name in ("u8_128_m70", "i8_64_m16", "f32_128_m32", "u8_48", "f32_320"):
        out.append(Case("search_exact", name, "exact", ("graph",), _opt(layout=0)))
        out.append(Case("search_exact", name, "exact", ("vectors",), _opt(layout=1)))
    out.append(Case("search_exact", "f32_128_m32", "fp16_exact", ("vectors",), _opt(layout=1, f16=1)))
    for name in ("u8_128_m70", "f32_128_m32"):
        for W in (2, 4):
            out.append(Case("search_exact_beam", name, f"beam{W}", ("graph",), _opt(layout=0)))
            out.append(Case("search_exact_beam", name, f"beam{W}", ("vectors",), _opt(layout=1)))
    out.append(Case("search_lut", "u8_130_m13", "base", ("graph", "codes")))
    out.append(Case("search_lut", "f32_128_m32", "base", ("graph", "codes"), _opt(lut=1)))
    for name in ("u8_128_m70", "u8_128_m32", "f32_96_m74", "i8_64_m16"):
        for entry, mode in (("search", "base"), ("search_inmem", "inmem"), ("search_wf", "wf")):
            out.append(Case(entry, name, mode, ("graph", "codes", "vectors")))
    out.append(Case("front_back", "u8_128_m70", "base", ("codes",)))
    out.append(Case("pqdist_stream", "u8_128_m70", "base", ("codes",)))
    for name in ("u8_128_m70", "f32_96_m74", "f32_320", "u8_130_m13"):
        out.append(Case("rerank", name, "base", ("vectors",)))
    for name in ("f32_100", "f32_260"):
        out.append(Case("rerank_f16", name, "fp16_base", ("vectors",), _opt(f16=1)))
    for o in (dict(search=1), dict(filter_layout=1), dict(semantics=1), dict(graph=0, pull=1)):
        mode = "wf" if "filter_layout" in o else "inmem" if "semantics" in o else "base"
        out.append(Case("engine", "u8_128_m70", mode, ("codes",), _opt(**o)))
    out.append(Case("engine", "u8_130_m13", "base", ("codes",), _opt(search=1)))
    return out


CASES = _cases()


def case_id(c: Case) -> str:
    return "-".join([c.entry, c.input, c.mode, "+".join(c.tables)] + [f"{k}{v}" for k, v in c.opt])


def vectors_in_graph(c: Case) -> bool:
    """The stretched "vectors" of this case are the vector part of the stretched graph entries (rr_vec_base = d_graph, vec_stride = entry_len)."""
    return c.entry in ("search", "search_inmem", "search_wf", "rerank")


def stride_for(c: Case, which: str) -> int:
    return stride_of(compact_stride(c.input, which, fp16=bool(dict(c.opt).get("f16")), vectors_in_graph=vectors_in_graph(c)))


def cpu_params():
    """(input, table, mode, stride, fp16) of every stretched table of every case, each once.  A case that stretches the graph entries of an
    exact-distance walk reads the vectors there too, by an address expression of its own: both tables are asked for."""
    seen = []
    for c in CASES:
        tables = c.tables + (("vectors",) if c.mode.startswith(("exact", "beam")) and c.tables == ("graph",) else ())
        for which in tables:
            stride = stride_of(compact_stride(c.input, "graph")) if which == "vectors" and "graph" in tables else stride_for(c, which)
            p = (c.input, which, c.mode, stride, bool(dict(c.opt).get("f16")))
            if p not in seen:
                seen.append(p)
    return seen


# ------------------------------------------------------------------------------------------------------------------------ the entries without a walk
LOG_BLOW = 16 << 20                   # the vector logs have L + 50 rows of Q slots: 16 MiB apart they reach 21.75 GiB
CONVERT_D = (7, 96)


def pqdist_lists():
    """bang_k_pqdist_stream: per query 1 .. 64 distinct ids of the N."""
    rng = np.random.default_rng(77)
    return [rng.choice(N, int(rng.integers(1, 65)), replace=False).astype(np.uint32) for _ in range(Q)]


def log_stride(ix) -> int:
    return LOG_BLOW + ix.D * tsize(ix)


def log_rows(n: int) -> np.ndarray:
    """by_row form: the iteration row of candidate i of a log of n entries.  Row 0 is the medoid's (read from d_medoid_vec, not from the log);
    the others count DOWN from the last row, so that the first candidates -- which every query has -- are the ones furthest out."""
    r = (L + 50) - np.arange(n, dtype=np.int64)
    r[0] = 0
    return r


def log_slots(logs, form: str):
    """Per query, the slot (in units of vec_stride) of the vector of candidate 1, 2, ... of its log: by_row (bang_k_rerank with d_cand_row):
    row * Q + q; by_query (bang_k_rerank_byquery): q * (L + 50) + i.  Candidate 0 is the medoid and has no slot."""
    if form == "by_row":
        return [log_rows(len(log))[1:] * Q + i for i, log in enumerate(logs)]
    assert form == "by_query"
    return [i * (L + 50) + np.arange(1, len(log), dtype=np.int64) for i, log in enumerate(logs)]


def rerank_of_slots(ix, q, logs, slots, table):
    """K6 + K7 on the CPU with candidate i >= 1 of query j's log read from table[slots[j][i - 1]] and candidate 0 from the medoid's entry."""
    import ctypes as C
    from oracle import oracle as O
    fn = O.lib().orc_exact_dist
    t = np.ascontiguousarray(table)
    ids, dists = np.empty((Q, K), np.uint64), np.empty((K, Q), np.float32)
    for j, log in enumerate(logs):
        rows = [np.ascontiguousarray(ix.graph[int(log[0]), :t.shape[1]])] + [t[int(s)] for s in slots[j]]
        v = np.ascontiguousarray(q[j])
        d = np.array([fn(C.c_void_p(r.ctypes.data), C.c_void_p(v.ctypes.data), C.c_uint32(ix.D), C.c_int(O.DTYPE_CODE[ix.dtype]), C.c_int(0)) for r in rows],
                     np.float32)
        ids[j], dists[:, j] = O.topk(log, d, K)
    return ids, dists


def convert_rows(D: int) -> np.ndarray:
    """float32 [N][D] for bang_k_f32_to_f16, no value of which rounds to a zero half."""
    rng = np.random.default_rng(900 + D)
    x = (rng.standard_normal((N, D)) * 100.0).astype(np.float32)
    x[np.abs(x) < 1e-3] = 1.0
    return x
