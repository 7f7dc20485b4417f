"""Small deterministic indexes with the layouts option ``any_dim`` adds to the exact-distance search mode, one per place where the any-dimension kernel can go
wrong.  TEST INFRASTRUCTURE ONLY (a helper module, not a conftest) of tests/test_anydim_inputs.py (CPU: the inputs) and tests/test_gpu_anydim.py (the kernel)."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from bang_amd import synth
from bang_amd.formats import NP_DTYPE, pack_graph
from exact_reference import Reference
from oracle import oracle as O

Q = 8
KL = ((10, 10), (10, 37))
# name -> (N, D, dtype, R, m, query elements dropped at the end: 1 = MIPS)
TABLE = {
    "u8_100":       (300, 100,  "uint8", 32, 25,  0),   # P = 7 pieces under G = 8 lanes, tail of one dword
    "i8_100":       (300, 100,  "int8",  32, 25,  0),   # the same, signed: the SPACEV1B row
    "u8_20":        (300, 20,   "uint8", 16, 5,   0),   # G = 2, tail of 4 bytes
    "u8_20_mips":   (300, 20,   "uint8", 16, 5,   1),   # u8_20 with queries of 19 bytes: a query row that starts at any address
    "u8_4":         (200, 4,    "uint8", 16, 2,   0),   # one dword, G = 1
    "u8_260":       (300, 260,  "uint8", 32, 65,  0),   # tile path, tail of one dword just past 256
    "i8_1020_far":  (200, 1020, "int8",  16, 255, 0),   # tile path; base in [-128, -118), queries in [118, 128): past 2^24, the float chain over a tail
    "f32_5":        (300, 5,    "float", 16, 2,   0),   # one piece plus a tail of 1
    "f32_67":       (300, 67,   "float", 32, 17,  0),   # crosses the 64-element query register, tail of 3
    "f32_201_mips": (300, 201,  "float", 32, 67,  1),   # queries of 200 floats (text2image after the MIPS transform)
    "f32_257":      (200, 257,  "float", 16, 65,  0),   # tile path, tail of 1
    "f32_1023":     (200, 1023, "float", 16, 256, 0),   # tile path, tail of 3
    "f32_96_mips":  (300, 96,   "float", 32, 24,  1),   # an aligned layout whose only new thing is the query stride
}
NAMES = tuple(TABLE)


def is_mips(name: str) -> bool:
    return name in TABLE and TABLE[name][5] != 0


@functools.lru_cache(maxsize=None)
def get(name: str):
    N, D, dtype, R, m, drop = TABLE[name]
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=4, seed=5000 + D + R, device="cpu", pq_iters=1)
    if name == "i8_1020_far":                              # (the PQ side of the index is left as it is: this input is for the exact mode only)
        rng = np.random.default_rng(6000 + D)
        q = rng.integers(118, 128, q.shape).astype(NP_DTYPE[dtype])
        ix = dataclasses.replace(ix, graph=pack_graph(rng.integers(-128, -118, (N, D)).astype(NP_DTYPE[dtype]), ix.degrees(), ix.adjacency()))
    return ix, np.ascontiguousarray(q[:, :D - drop])


class MipsReference(Reference):                            # queries without the last coordinate: orc_exact_dist with dim_adjust = 1 reads it as 0
    def exact(self, ids, query):
        fn, qp = O.lib().orc_exact_dist, C.c_void_p(query.ctypes.data)
        return np.array([fn(C.c_void_p(self._gbase + int(x) * self._entry_len), qp, C.c_uint32(self.ix.D), self._dcode, C.c_int(1)) for x in ids], np.float32)


@functools.lru_cache(maxsize=None)
def reference(name: str, k: int, L: int):
    ix, q = get(name)
    return (MipsReference if is_mips(name) else Reference)(ix).search(q, k, L, "exact")
