"""tests/float_range_inputs.py reaches the edges it is named for -- asserted on the CPU references alone -- and bang_check_floats, the host check
of the float input domain (CANON 20), accepts and refuses what it must: through ctypes, and once more as a stand-alone C
program built with the check's translation unit under -fsanitize=address,undefined (no Python runs under a sanitizer).

Measured here (printed with -s): the exponents chosen per base index and the shares of top-10 exact distances that are subnormal / zero there:

    base       subnormal e  share subnormal   zero e   share zero
    d68           -69           1.00           -79       1.00
    d252          -70           1.00           -80       1.00
    d4            -66           1.00           -77       1.00
    f32_260       -70           1.00           -80       1.00
    fp16_256      -70           1.00           -80       1.00
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import float_range_inputs as FR
import labels_inputs as LI
import labels_reference as LR
import range_reference as RR
from beam_reference import Reference as BeamReference
from exact_reference import BIG_DIST, Reference as ExactReference
from inmemory_reference import Reference as InmemReference
from wordfilter_reference import Reference as WordReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bang-billion-scale-ann_amd", "csrc")
K = FR.K
ERR_ARG = -1
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _runs(name, what, L):
    """Every reference on one input at one L: {reference: (ids, dists, counters, candidate logs or None)}; once per (base, input, L)."""
    key = (name, what, L)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import oracle as O
    ix, q = FR.get(name, what)
    Q = q.shape[0]
    out = {}
    out["oracle_l2"] = O.Oracle(ix).search(q, K, L, with_stats=True) + (None,)
    out["oracle_mips"] = O.Oracle(ix).search(np.ascontiguousarray(q[:, :-1]), K, L, mips=True, with_stats=True) + (None,)     # (MIPS queries: D - 1)
    out["exact"] = ExactReference(ix).search(q, K, L, "exact") + (None,)
    im = InmemReference(ix)
    for mode in ("base", "inmemory"):
        rows = [im.search_one_logged(q[i], K, L, mode) for i in range(Q)]
        out[mode] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows], axis=1), np.array([r[2] for r in rows], np.int64), [r[3] for r in rows])
    wf = WordReference(ix)
    rows, logs = [], []
    for i in range(Q):
        log = []
        rows.append(wf.search_one(q[i], K, L, "word", log=log))
        logs.append(np.array(log, np.uint32))
    out["wordfilter"] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows], axis=1), np.array([r[2] for r in rows], np.int64), logs)
    ids, d, st, log = BeamReference(ix).search(q, K, L, 2)
    out["beam2"] = (ids, d, st, [np.asarray(x) for x in log])
    tr = LR.Reference(ix).walks(q, L)
    any_, all_ = LI.batch("all2", Q)
    ids, d, matched, st, _ = LR.collect_all(tr, LI.rand4(ix.N), any_, all_, K, L, int(ix.medoid))
    out["labels"] = (ids, d, np.concatenate([st, matched[:, None].astype(np.int64)], axis=1), [t.log for t in tr])
    rt = RR.Reference(ix).evaluated_all(q, L)
    out["range_traces"] = rt
    lims, ids, d, counts, offered = RR.collect_all(rt, np.full(Q, np.inf, np.float32), 512)
    out["range"] = (ids, d, np.stack([lims[1:].astype(np.int64), counts.astype(np.int64), offered.astype(np.int64)] +
                                     [np.array([t.stats[j] for t in rt], np.int64) for j in range(4)], axis=1), [t.log for t in rt])
    _CACHE[key] = out
    return out


REFERENCES = ("oracle_l2", "oracle_mips", "exact", "base", "inmemory", "wordfilter", "beam2", "labels", "range")


def _same_logs(a, b):
    return (a is None and b is None) or (len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)))


@pytest.mark.parametrize("L", FR.LS)
@pytest.mark.parametrize("scale", FR.INVARIANT)
@pytest.mark.parametrize("name", FR.BASES)
def test_up_and_down_leave_ids_and_shift_exponents(name, scale, L):
    """Oracle.search (L2 and MIPS), the exact, Inmemory, word-filter, beam, labels and range references: ids, counters and candidate logs of the
    unscaled index, every distance's bits those of the unscaled distance times 2^(2e)."""
    e = FR.exp_of(name, scale)
    want, got = _runs(name, "unscaled", L), _runs(name, scale, L)
    for r in REFERENCES:
        assert np.array_equal(got[r][0], want[r][0]), (r, "ids")
        assert np.array_equal(got[r][2], want[r][2]), (r, "counters")
        assert _same_logs(got[r][3], want[r][3]), (r, "candidate log")
        assert np.array_equal(_bits(got[r][1]), FR.shifted_bits(want[r][1], e)), (r, "distance bits")
        real = want[r][1] != BIG_DIST                                                      # (not the padding sentinel)
        assert real.any() and not FR.is_subnormal(got[r][1][real]).any(), r                   # nothing underflowed:
        assert np.array_equal(got[r][1][real] == 0, want[r][1][real] == 0), r                 # a zero was a zero before


@pytest.mark.parametrize("name", FR.BASES)
def test_subnormal_scale_reaches_subnormal_distances(name):
    ix, q = FR.get(name, "subnormal")
    t = FR.top10_exact(ix, q)
    share = float(FR.is_subnormal(t).mean())
    print(f"\n{name}: subnormal e = {FR.subnormal_exp(name)}, share of top-10 exact distances subnormal {share:.2f}, zero {float((t == 0).mean()):.2f}")
    assert share >= 0.5
    v = np.concatenate([a.reshape(-1) for a in (ix.vectors(), ix.pivots, ix.centroid, q)])
    assert not FR.is_subnormal(v).any() and (v != 0).mean() > 0.99                       # the values themselves stay normal
    # ... and rounding in the subnormal range changes the walk: ids differ from the unscaled run, or tie where they did not
    changed = False
    for L in FR.LS:
        a, b = _runs(name, "unscaled", L)["exact"], _runs(name, "subnormal", L)["exact"]
        ties_a, ties_b = (a[1][1:] == a[1][:-1]).any(axis=0), (b[1][1:] == b[1][:-1]).any(axis=0)
        changed |= bool((a[0] != b[0]).any(axis=1).any() or (ties_b & ~ties_a).any())
        assert FR.is_subnormal(b[1]).mean() >= 0.5 and np.isfinite(b[1]).all()
    assert changed


@pytest.mark.parametrize("name", FR.BASES)
def test_zero_scale_underflows_every_distance(name):
    ix, q = FR.get(name, "zero")
    t = FR.top10_exact(ix, q)
    print(f"\n{name}: zero e = {FR.zero_exp(name)}, share of top-10 exact distances zero {float((t == 0).mean()):.2f}")
    v = np.concatenate([a.reshape(-1) for a in (ix.vectors(), ix.pivots, ix.centroid, q)])
    assert not FR.is_subnormal(v).any() and (v != 0).mean() > 0.99
    zero = np.uint32(0)                                                                   # +0: not -0
    assert (_bits(FR._all_exact(ix, q)) == zero).all() and (_bits(FR._all_pq(ix, q)) == zero).all()
    for L in FR.LS:
        runs = _runs(name, "zero", L)
        for t_ in runs["range_traces"]:
            assert all((_bits(d) == zero).all() for _, _, d in t_.iters)
        for r in REFERENCES:
            d = runs[r][1]
            assert (_bits(d[d != BIG_DIST]) == zero).all(), r


@pytest.mark.parametrize("name", FR.BASES)
def test_signed_input(name):
    ix, q = FR.get(name, "signed")
    v = ix.vectors()
    assert (v < 0).mean() >= 0.30
    assert (_bits(v) == np.uint32(0x80000000)).any() and (_bits(q) == np.uint32(0x80000000)).any()      # -0.0
    copies = [int(np.flatnonzero((_bits(v) == _bits(q[i])[None, :]).all(axis=1)).size) for i in (0, 1)]
    assert copies[0] >= 3 and copies[1] >= 2                                                          # bit-copies: 2 queries, 3 duplicates
    for L in FR.LS:
        d = _runs(name, "signed", L)["exact"][1]
        assert (_bits(d[0, :2]) == 0).all()                                                           # a result at exactly +0 ...
        assert (_bits(d[1, :2]) == 0).any()                                                           # ... and a zero tie in one query's top 10
        assert (_bits(_runs(name, "signed", L)["oracle_l2"][1]) == 0).any()                           # (the re-rank of the PQ walk meets one too)


@pytest.mark.parametrize("name", FR.BASES)
def test_offset_input(name):
    ix, q = FR.get(name, "offset")
    v = ix.vectors()
    assert v.min() >= 2.0 ** 20 - 2 and v.max() <= 2.0 ** 20 + 2 and np.array_equal(v, np.round(v * 16) / 16)     # ulp 1/8 above 2^20, 1/16 below
    d = _runs(name, "offset", 37)["exact"][1]
    assert np.isfinite(d).all() and d.max() < 1e4


@pytest.mark.parametrize("what", FR.NAMES + ("fp16_straddle",))
@pytest.mark.parametrize("name", FR.BASES)
def test_every_input_is_inside_the_domain(name, what):
    """Every value within |x| <= 2^56, and the largest EVALUATED distance (the range reference's traces) finite and below BIG_DIST."""
    ix, q = FR.get(name, what)
    assert FR.in_domain(ix, q)
    for a in (ix.vectors(), ix.pivots, ix.centroid, q):
        assert _check(a.reshape(-1))[0] == 0
    if what == "fp16_straddle":
        traces = RR.Reference(ix).evaluated_all(q, 37)
    else:
        traces = _runs(name, what, 37)["range_traces"]
    dmax = max(float(d.max()) for t in traces for _, _, d in t.iters)
    assert np.isfinite(dmax) and dmax < float(BIG_DIST)
    if what == "up":
        assert dmax > 2.0 ** 80


def test_fp16_straddle_is_on_both_sides_of_the_smallest_normal_half():
    import fp16_inputs as FP
    ix, q = FR.get("fp16_256", "fp16_straddle")
    v = np.abs(ix.vectors())
    below = float(((v < 2.0 ** -14) & (v > 0)).mean())
    assert 0.25 <= below <= 0.75, below
    h = ix.vectors().astype(np.float16)
    sub = (h.view(np.uint16) & 0x7C00) == 0
    assert 0.25 <= float(sub.mean()) <= 0.75 and np.isfinite(h.astype(np.float32)).all()
    a = FP.exact_reference(("fr", "straddle"), ix, q, K, 37)
    b = FP.exact_reference(("fr", "straddle", "rounded"), FP.rounded(ix), q, K, 37)
    assert FP.distance_bits_differ(a, b)                                                  # the rounded table is not the float one


# ---------------------------------------------------------------------------------------------------------------------
# bang_check_floats
# ---------------------------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


TWO56 = np.float32(2.0 ** 56)
REFUSED = [_f(0x7FC00000), _f(0xFFC00000), _f(0x7F800001), _f(0xFFFFFFFF), _f(0x7FA5A5A5), np.float32(np.inf), np.float32(-np.inf),
           np.nextafter(TWO56, np.float32(np.inf)), -np.nextafter(TWO56, np.float32(np.inf)), np.float32(2.0 ** 57), np.float32(3.402823e38)]
ACCEPTED = [TWO56, -TWO56, _f(0x00000001), _f(0x807FFFFF), _f(0x00400000), np.float32(0.0), np.float32(-0.0), np.float32(1.0), np.float32(-128.0),
            np.nextafter(TWO56, np.float32(0))]


def _check(a):
    """-> (rc, first_bad or None)"""
    from bang_amd import binding as B
    fn = B.lib().bang_check_floats
    fn.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    a = np.ascontiguousarray(a, np.float32)
    bad = C.c_uint64(0xDEADBEEF)
    rc = fn(a.ctypes.data if a.size else None, a.size, C.byref(bad))
    return rc, (None if bad.value == 0xDEADBEEF else int(bad.value))


def test_check_through_ctypes():
    assert np.nextafter(TWO56, np.float32(np.inf)).view(np.uint32) == 0x5B800001 and TWO56.view(np.uint32) == 0x5B800000
    assert _check(np.zeros(0, np.float32)) == (0, None)                                   # n = 0
    acc = np.array(ACCEPTED, np.float32)
    for n in list(range(1, 68)) + [1024, 1025, 4099]:
        clean = np.resize(acc, n)
        assert _check(clean) == (0, None), n
        for r in REFUSED:
            for at in sorted({0, n // 2, n - 1}):
                x = clean.copy()
                x[at] = r
                assert _check(x) == (ERR_ARG, at), (n, r, at)
                x[n - 1] = REFUSED[0]                                                     # a second offender behind: the FIRST is reported
                assert _check(x) == (ERR_ARG, at), (n, r, at)


def test_numpy_check_agrees_with_the_library():
    from bang_amd import formats
    for v in ACCEPTED:
        formats.check_floats("t", np.array([[1.0, v]], np.float32))
    for v in REFUSED:
        with pytest.raises(ValueError, match=r"t: element \(2, 1\)"):
            formats.check_floats("t", np.array([[1.0, 2.0], [1.0, v]], np.float32), row0=1)


@pytest.mark.parametrize("dtype", ["uint8", "float"])
def test_write_index_refuses_values_outside_the_domain(dtype, tmp_path, request):
    """formats.write_index validates pivots and centroid of any index and the vectors of a float one, and writes nothing."""
    import dataclasses
    from bang_amd import formats
    ix = request.getfixturevalue("small_u8" if dtype == "uint8" else "small_f32")[0]
    piv = ix.pivots.copy()
    piv[255, ix.D - 1] = np.nan
    cen = ix.centroid.copy()
    cen[0] = np.inf
    bad = [("pivot", dataclasses.replace(ix, pivots=piv)), ("centroid", dataclasses.replace(ix, centroid=cen))]
    if dtype == "float":
        g = ix.graph.copy()
        g[ix.N - 1, 4 * (ix.D - 1): 4 * ix.D] = np.array([np.nan], np.float32).view(np.uint8)
        bad.append(("vectors", dataclasses.replace(ix, graph=g)))
    for what, b in bad:
        prefix = str(tmp_path / what / "ix")
        with pytest.raises(ValueError, match="finite") as ei:
            formats.write_index(prefix, b)
        assert what in str(ei.value)
        assert not os.path.exists(os.path.dirname(prefix))
    formats.write_index(str(tmp_path / "ok" / "ix"), ix)


def test_check_under_sanitizers(tmp_path):
    """csrc/bang_check.cpp + tests/check_floats_main.cpp built with -fsanitize=address,undefined and run: the cases above in C, every buffer
    heap-allocated to exactly n floats."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "check_floats_san")
    # (the runtimes linked into the program: it is self-contained, whatever else the loader brings)
    cmd = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "bang_check.cpp"),
           os.path.join(ROOT, "tests", "check_floats_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")                 # (leak checking needs ptrace; the cases are about reads)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 67 * 3 * len(REFUSED)
