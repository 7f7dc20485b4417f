"""Records what the host side of the search kernel answers (python tests/golden/make_search_host_golden.py [path/to/libbang.so]).

Pure host functions of libbang -- which PQ layout an index gets, how its pivot table is packed, which instances exist, the launch geometry --
asked over a fixed list of arguments; the answers, error codes included, go to tests/golden/search_host_sweep.json.  The committed file was
written from the library of the commit BEFORE these functions moved from csrc/bang_search.hip and csrc/bang_kernels.hip to
csrc/bang_search_host.cpp, on a machine without a GPU, where bang_num_cus answers 256 (an MI355X has 256 too).
tests/test_search_host.py::test_the_library_reproduces_the_recorded_sweep asks the tree's library the same questions and compares exactly.

bang_search_geometry: the full product of the values below is 64 512 rows.  Recorded are layouts x L x Q of either pacing form with (nctx,
group_waves, caps) cycling through all 48 triples, shifted per layout; all Q x caps of the self-paced form at L = 152; and all 48 triples of the
host-paced form at L = 152, Q = 10 000 -- for every layout.  4 739 rows over all functions.

The file holds, per function, the answers in the order sweep() asks and a digest of the questions (so that a change of the list below is told apart
from a change of an answer): a question is not stored, sweep() makes it again."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "bang-billion-scale-ann_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "search_host_sweep.json")
LAYOUTS = ((1, 8), (1, 16), (1, 24), (1, 32), (2, 8), (2, 16), (2, 18), (2, 19), (4, 4), (4, 8), (8, 2), (8, 4))      # (psz, code dwords per row)
RAGGED = {(2, 18): (58, 70, 128), (2, 19): (22, 74, 96)}                                                             # -> nhi, m, D
TABLES = [(psz, 4 * ndw, 0) for psz, ndw in LAYOUTS] + [(psz, 4 * ndw, RAGGED[psz, ndw][0]) for psz, ndw in RAGGED]  # (psz, mp, nhi): 12 + 2
LS = (1, 37, 152, 161, 162, 512)
QS = (1, 255, 256, 257, 1280, 1281, 4000, 10000)
NCTX, GROUP_WAVES, CAPS = (0, 1, 2, 3), (0, 2, 8, 32), ((0, 0), (96, 0), (0, 3))
U32 = C.c_uint32


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _geometry(lib, psz, mp, nhi, L, Q, max_wgs, max_waves, host_paced, nctx, gw):
    wg, w, n, g = U32(0), U32(0), U32(nctx), U32(gw)
    rc = lib.bang_search_geometry(psz, mp, nhi, L, Q, max_wgs, max_waves, host_paced, C.byref(wg), C.byref(w), C.byref(n), C.byref(g))
    return [rc, wg.value, w.value, n.value, g.value] if rc == 0 else [rc]


def _geometry2(f, psz, mp, nhi, L, Q, max_wgs, max_waves):
    wg, w = U32(0), U32(0)
    rc = f(psz, mp, nhi, L, Q, max_wgs, max_waves, C.byref(wg), C.byref(w))
    return [rc, wg.value, w.value] if rc == 0 else [rc]


def _pivots(D, seed):
    return np.random.default_rng(seed).normal(size=(256, D)).astype(np.float32)


def _pack(lib, chunk_off, D, m, psz, mp):
    piv, out = _pivots(D, 1000 * psz + mp), np.full(mp * 256 * psz, 7.0, np.float32)
    rc = lib.bang_pack_pivots(piv.ctypes.data, chunk_off.ctypes.data, D, m, psz, mp, out.ctypes.data)
    return [rc, _digest(out)]


def _pack_ragged(lib, chunk_off, D, m, mp):
    piv, nhi, nfl = _pivots(D, 2000 + mp), U32(99), C.c_uint64(99)
    rc = lib.bang_pack_pivots_ragged(None, chunk_off.ctypes.data, D, m, mp, C.byref(nhi), None, C.byref(nfl))      # the size query
    row = [rc, nhi.value, nfl.value]
    if rc == 0 and nhi.value:
        out = np.full(nfl.value, 7.0, np.float32)
        row += [lib.bang_pack_pivots_ragged(piv.ctypes.data, chunk_off.ctypes.data, D, m, mp, C.byref(nhi), out.ctypes.data, C.byref(nfl)), _digest(out)]
    return row


def _rerank_layouts():
    """the dtype x D x stride grid of tests/test_instance_inputs.py::test_the_restated_layout_rule_is_the_librarys"""
    import base_forms as F
    import edge_inputs as E
    import instance_inputs as I
    from oracle import oracle as O
    layouts = {(e.dtype, e.D, e.R) for e in I.ENTRIES} | {(s[2], s[1], s[3]) for s in E.SHAPES} | {(t, D, 64) for t, D in E.TOY_LAYOUTS}
    layouts |= {(t, D, 64) for t in ("uint8", "int8", "float") for D in (1, 3, 4, 15, 16, 17, 48, 96, 250, 256, 260, 272, 512)}
    for dtype, D, R in sorted(layouts):
        for stride in (D * F.tsize(dtype), D * F.tsize(dtype) + 4 + 4 * R):
            yield O.DTYPE_CODE[dtype], D, stride


def sweep(lib):
    """{function: rows}; a row is the arguments followed by the answer"""
    lib.bang_pq_layout.argtypes = [C.c_void_p, U32, U32, C.POINTER(U32), C.POINTER(U32)]
    lib.bang_pack_pivots.argtypes = [C.c_void_p, C.c_void_p, U32, U32, U32, U32, C.c_void_p]
    lib.bang_pack_pivots_ragged.argtypes = [C.c_void_p, C.c_void_p, U32, U32, U32, C.POINTER(U32), C.c_void_p, C.POINTER(C.c_uint64)]
    lib.bang_ragged_supported.argtypes = lib.bang_search_supported.argtypes = [U32] * 4
    lib.bang_search_geometry.argtypes = [U32] * 7 + [C.c_int] + [C.POINTER(U32)] * 4
    lib.bang_search_inmem_geometry.argtypes = lib.bang_search_wf_geometry.argtypes = [U32] * 7 + [C.POINTER(U32)] * 2
    lib.bang_search_inmem_has_instance.argtypes = lib.bang_search_wf_has_instance.argtypes = [U32] * 3
    lib.bang_search_can_rerank.argtypes = [C.c_int, U32, C.c_uint64, U32]
    out = {"cus": lib.bang_num_cus()}

    rows = []
    for width, m in itertools.product((1, 2, 3, 4, 5, 8, 9), range(1, 133)):
        off, psz, mp = np.arange(m + 1, dtype=np.uint32) * width, U32(77), U32(77)
        rows.append([width, m, lib.bang_pq_layout(off.ctypes.data, width * m, m, C.byref(psz), C.byref(mp)), psz.value, mp.value])
    off = np.array([0, 2, 1, 3], np.uint32)                                       # descending offsets
    rows.append(["bad", 3, lib.bang_pq_layout(off.ctypes.data, 3, 3, C.byref(psz), C.byref(mp)), psz.value, mp.value])
    out["pq_layout"] = rows

    rows = []
    for psz, ndw in LAYOUTS:                                                       # uniform chunks of psz dims, two padding chunks
        mp, m = 4 * ndw, 4 * ndw - 2
        rows.append([psz, mp, m] + _pack(lib, np.arange(m + 1, dtype=np.uint32) * psz, psz * m, m, psz, mp))
    ragged = [(nhi, m, D, 4 * ndw) for (_, ndw), (nhi, m, D) in RAGGED.items()] + [(40, 60, 100, 64)]     # the last: packed, but no instance
    for nhi, m, D, mp in ragged:
        off = np.concatenate([np.arange(nhi + 1) * 2, 2 * nhi + 1 + np.arange(m - nhi)]).astype(np.uint32)
        rows.append(["ragged", mp, m] + _pack_ragged(lib, off, D, m, mp) + [lib.bang_ragged_supported(2, mp, nhi, m)])
        rows.append(["padded", mp, m] + _pack(lib, off, D, m, 2, mp))
    off = np.array([0, 2, 4, 7, 8], np.uint32)                                     # 2, 2, 3, 1: no exact-size form
    rows.append(["ragged", 8, 4] + _pack_ragged(lib, off, 8, 4, 8))
    rows.append(["ragged", 3, 4, lib.bang_pack_pivots_ragged(None, off.ctypes.data, 8, 4, 3, C.byref(U32()), None, None)])      # mp < m
    out["pack_pivots"] = rows

    out["ragged_supported"] = [[psz, mp, nhi, m, lib.bang_ragged_supported(psz, mp, nhi, m)]
                               for psz, mp, nhi, m in itertools.product((1, 2, 4), (64, 72, 76, 80), (0, 22, 40, 58), (60, 70, 72, 74, 76))]

    out["search_supported"] = [[psz, mp, nhi, L, lib.bang_search_supported(psz, mp, nhi, L)]
                               for (psz, mp, nhi), L in itertools.product(TABLES + [(0, 32, 0), (2, 80, 0)], LS + (0, 513))]

    rows, triples = [], list(itertools.product(NCTX, GROUP_WAVES, CAPS))

    def ask(psz, mp, nhi, L, Q, host_paced, nctx, gw, caps):
        rows.append([psz, mp, nhi, L, Q, *caps, host_paced, nctx, gw] + _geometry(lib, psz, mp, nhi, L, Q, *caps, host_paced, nctx, gw))
    for t, table in enumerate(TABLES):
        for host_paced in (0, 1):
            for i, (L, Q) in enumerate(itertools.product(LS, QS)):
                ask(*table, L, Q, host_paced, *triples[(i + 7 * t + 24 * host_paced) % 48])
        for Q, caps in itertools.product(QS, CAPS):
            ask(*table, 152, Q, 0, 0, 0, caps)
        for nctx, gw, caps in triples:
            ask(*table, 152, 10000, 1, nctx, gw, caps)
    for bad in ((0, 32, 0, 152, 100), (2, 72, 0, 0, 100), (2, 72, 0, 513, 100), (2, 72, 0, 152, 0), (2, 80, 0, 512, 100)):
        ask(*bad, 0, 0, 0, (0, 0))
    out["search_geometry"] = rows

    for name in ("bang_search_inmem_geometry", "bang_search_wf_geometry"):
        f = getattr(lib, name)
        out[name[5:]] = [[psz, mp, nhi, L, Q, wgs, waves] + _geometry2(f, psz, mp, nhi, L, Q, wgs, waves)
                         for i, ((psz, mp, nhi), L, Q) in enumerate(itertools.product(TABLES + [(0, 32, 0)], (1, 152, 512), QS)) for wgs, waves in (CAPS[i % 3],)]

    keys = [(psz, 4 * ndw) for psz, ndw in LAYOUTS] + [(0, 32), (1, 48), (2, 80), (2, 74), (3, 32), (4, 32), (8, 32)]
    for name in ("bang_search_inmem_has_instance", "bang_search_wf_has_instance"):
        out[name[5:]] = [[psz, mp, stride, getattr(lib, name)(psz, mp, stride)] for psz, mp in keys for stride in (mp, mp - 2)]

    out["search_can_rerank"] = [[t, D, stride, adj, lib.bang_search_can_rerank(t, D, stride, adj)]
                                for t, D, stride in _rerank_layouts() for adj in (0, 1)] + [[3, 128, 128, 0, lib.bang_search_can_rerank(3, 128, 128, 0)]]
    return out


# arguments in front of a row's answer
NARGS = {"pq_layout": 2, "pack_pivots": 3, "ragged_supported": 4, "search_supported": 4, "search_geometry": 10, "search_inmem_geometry": 7,
         "search_wf_geometry": 7, "search_inmem_has_instance": 3, "search_wf_has_instance": 3, "search_can_rerank": 4}


def record(out):
    """what the file holds: per function a digest of the questions and the answers alone (a single number where the answer is one)"""
    rec = {"cus": out["cus"]}
    for name, n in NARGS.items():
        answers = [r[n:] for r in out[name]]
        rec[name] = {"questions": hashlib.sha256(json.dumps([r[:n] for r in out[name]]).encode()).hexdigest()[:16],
                     "answers": [a[0] if len(a) == 1 else a for a in answers]}
    return rec


def dump(out, path):
    with open(path, "w") as f:                                                    # one function per line
        f.write("{\n" + ",\n".join(f'"{k}": ' + json.dumps(v, separators=(",", ":")) for k, v in record(out).items()) + "\n}\n")


if __name__ == "__main__":
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bang-billion-scale-ann_amd", "lib", "libbang.so")
    result = sweep(C.CDLL(so))
    dump(result, OUT)
    print(so, {k: (len(v) if isinstance(v, list) else v) for k, v in result.items()}, sum(len(v) for v in result.values() if isinstance(v, list)), "rows")
