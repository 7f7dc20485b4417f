"""The inputs of tests/anydim_inputs.py reach the ground they are named for, on the CPU (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import anydim_inputs as A


@pytest.mark.parametrize("name", A.NAMES)
def test_input_reaches_the_ground_it_is_named_for(name, libbang):
    ix, q = A.get(name)
    any_fn, old_fn = libbang.bang_search_exact_anydim_supported, libbang.bang_search_exact_supported
    any_fn.argtypes = old_fn.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
    dt = ("uint8", "int8", "float").index(ix.dtype)                  # BANG_U8, BANG_I8, BANG_F32
    aligned = ix.D % (4 if ix.dtype == "float" else 16) == 0
    assert aligned == (name == "f32_96_mips") and q.shape == (A.Q, ix.D - (1 if A.is_mips(name) else 0))
    for stride in (ix.entry_len, ix.D * (4 if ix.dtype == "float" else 1)):
        assert any_fn(dt, ix.D, stride) == 1 and old_fn(dt, ix.D, stride) == (1 if aligned else 0)
    # (accepted with any_dim as graph entries and as a packed table, refused without where unaligned); 8-bit rows off the dword grid, D = 0, D > 1024 stay outside
    assert [any_fn(*a) for a in ((0, 42, 44), (1, 10, 12), (2, 0, 16), (2, 1025, 4100), (0, 100, 102))] == [0] * 5
    for k, L in A.KL:
        ids, d, st = A.reference(name, k, L)
        assert (st[:, 0] > 1).all() and (ids[:, 0] != np.iinfo(np.uint64).max).all()       # every walk runs more than one iteration
        assert name != "i8_1020_far" or (d > (1 << 24)).all()                                 # the far input leaves the integers a float holds
