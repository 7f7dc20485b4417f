"""One small index per compiled instance of the BANG_Base search kernel and per row alignment.

TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).  search_dispatch (csrc/bang_search.hip) switches on psz * 100 + mp / 4 over twelve
instances, and launch_al compiles each one twice: for code rows that start dword-aligned (code stride % 4 == 0) and for rows that do not.  The
fixtures and shape lists of the other files reach nine of the twelve, most of them in one alignment only; ENTRIES reaches every instance in both.
tests/test_instance_inputs.py asserts ON THE CPU that it does (bang_amd.binding.pq_layout) and that the reference walk on every layout gets past the
seed list; tests/test_gpu_search_instances.py runs every entry through every form of the walk.

    Entry          shape + the engine options that choose the variant: code_stride (0 = rows m bytes apart, else the stride in bytes; never -1,
                   which pads m = 70 / 74 / 90 ... to a power of two and so turns an unaligned case into an aligned one) and pq_ragged
                   (the exact-size pivot table of the 70- and 74-chunk layouts: offered / not offered)
    ENTRIES        the list;  entry_id(), stride_of(), aligned(), options_of(), runs_of()
    entry_index()  synth.make_index of an entry's shape, cached per SHAPE: entries that differ in the options only share index and references
"""
from __future__ import annotations

import collections
import functools

from bang_amd import synth

Entry = collections.namedtuple("Entry", "key N D dtype R m Q code_stride pq_ragged", defaults=(1,))

ENTRIES = [
    #     key  N    D    dtype    R   m    Q   code_stride
    # 1-dimension chunks (psz 1): m = D
    Entry(108, 600, 24,  "float", 32, 24,  12, 0),        # 6 code dwords, the fused re-rank (float, D % 4 == 0)
    Entry(108, 700, 30,  "uint8", 64, 30,  10, 0),        # rows 30 bytes apart; D % 16 != 0: the re-rank launch
    Entry(108, 700, 30,  "uint8", 64, 30,  10, 32),       # the same rows padded to a dword-aligned stride
    Entry(116, 640, 48,  "float", 64, 48,  10, 0),
    Entry(116, 560, 37,  "int8",  8,  37,  12, 0),        # a tiny degree bound, odd D
    Entry(124, 600, 80,  "float", 64, 80,  10, 0),        # 20 dwords: three groups of six and a tail of two
    Entry(124, 720, 90,  "uint8", 32, 90,  8,  0),        # 22.5 dwords
    Entry(124, 720, 90,  "uint8", 32, 90,  8,  92),
    Entry(132, 520, 128, "uint8", 64, 128, 8,  0),        # the widest row: all 32 dwords carry codes
    Entry(132, 640, 126, "float", 32, 126, 8,  0),        # (semantics = 1 has no instance for this one)
    Entry(132, 640, 126, "float", 32, 126, 8,  128),
    # 2-dimension chunks (psz 2)
    Entry(208, 600, 32,  "int8",  32, 16,  12, 0),
    Entry(208, 650, 50,  "float", 64, 25,  10, 0),
    Entry(216, 600, 128, "uint8", 64, 64,  8,  0),
    Entry(216, 700, 122, "float", 32, 61,  8,  0),
    # 2- and 1-dimension chunks: the SIFT1B-like and DEEP100M-like layouts of conftest.small_u8 / small_deep, packed and padded, with the
    # exact-size pivot table offered (pq_ragged 1: NHI = 58 / 22 where bang_alloc takes it) and not
    Entry(218, 700, 128, "uint8", 64, 70,  10, 0,   1),
    Entry(218, 700, 128, "uint8", 64, 70,  10, 0,   0),
    Entry(218, 700, 128, "uint8", 64, 70,  10, 128, 1),
    Entry(218, 700, 128, "uint8", 64, 70,  10, 128, 0),
    Entry(219, 640, 96,  "float", 64, 74,  10, 0,   1),
    Entry(219, 640, 96,  "float", 64, 74,  10, 0,   0),
    Entry(219, 640, 96,  "float", 64, 74,  10, 76,  1),
    Entry(219, 640, 96,  "float", 64, 74,  10, 76,  0),
    # 4-dimension chunks (psz 4)
    Entry(404, 600, 64,  "int8",  32, 16,  12, 0),
    Entry(404, 620, 24,  "uint8", 8,  6,   12, 0),        # rows of 6 bytes
    Entry(408, 600, 128, "float", 64, 32,  8,  0),
    Entry(408, 660, 68,  "uint8", 32, 17,  10, 0),
    # 5- to 8-dimension chunks (psz 8)
    Entry(802, 600, 64,  "uint8", 64, 8,   12, 0),
    Entry(802, 580, 40,  "int8",  32, 5,   12, 0),        # rows of 5 bytes
    Entry(802, 580, 40,  "int8",  32, 5,   12, 8),
    Entry(804, 700, 96,  "float", 64, 12,  10, 0),
    Entry(804, 640, 104, "int8",  8,  13,  10, 0),
]

NEVER_LAUNCHED_BEFORE = (108, 124, 802)      # no other file's layouts reach these keys
LAUNCH_SHAPE_KEYS = NEVER_LAUNCHED_BEFORE + (132,)      # the entries that also run the one-wave launch and the batches of 1, 7 and Q
RUNS = ((10, 10), (10, 37), (37, 37))        # (k, L) of every entry
LONG_L = 152                                 # one long worklist more ...


def has_long_run(e: Entry) -> bool:
    """... on the 124, 132 and 802 entries -- and on the 218 entries that offer the exact-size table: up to L = 37 the padded table leaves room
    for all 12 waves of that instance, so bang_alloc keeps it, and NHI = 58 would not run at all (test_instance_inputs pins both facts)."""
    return e.key in (124, 132, 802) or (e.key == 218 and e.pq_ragged == 1)


def runs_of(e: Entry):
    return RUNS + (((10, LONG_L),) if has_long_run(e) else ())


def stride_of(e: Entry) -> int:
    """Bytes between two code rows in HBM: what Stats.code_stride must report."""
    return e.code_stride if e.code_stride else e.m


def aligned(e: Entry) -> bool:
    return stride_of(e) % 4 == 0


def entry_id(e: Entry) -> str:
    return f"{e.key}-D{e.D}-{e.dtype}-R{e.R}-m{e.m}-cs{e.code_stride}" + ("" if e.pq_ragged else "-padded_table")


def shape_of(e: Entry):
    return e.N, e.D, e.dtype, e.R, e.m, e.Q


def options_of(e: Entry) -> dict:
    return dict(code_stride=e.code_stride, pq_ragged=e.pq_ragged)


@functools.lru_cache(maxsize=None)
def _shape_index(shape):
    N, D, dtype, R, m, Q = shape
    ix, q, _, _ = synth.make_index(N, D, dtype, R, m, Q, K=10, n_clusters=8, seed=3000 + N + D + R + m, device="cpu", pq_iters=2)
    return ix, q


def entry_index(e: Entry):
    """(index, queries) of an entry; treat both as read-only."""
    return _shape_index(shape_of(e))
