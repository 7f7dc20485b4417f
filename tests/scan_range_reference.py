"""CPU reference of the exact range scan (CANON 26).  TEST INFRASTRUCTURE ONLY (a helper module, not a conftest): a few lines of
numpy on tests/scan_reference.py -- its distances and candidate masks, the float compare, the first max_hits hits in id order, np.sort of the keys."""
import numpy as np

import scan_reference as SR


def answer(dist, radii, max_hits, n_nodes=None, **masks):
    """dist: float32 [Q][N] (scan_reference.distances); radii [Q]; masks: scan_reference.candidates' keywords.
    -> (lims u64 [Q + 1], ids u64, dists f32, offered u32 [Q], matched u32 [Q]), packed as Engine.scan_range returns them"""
    Q, N = dist.shape
    n = N if n_nodes is None else int(n_nodes)
    cand = SR.candidates(N, Q, **masks)[:, :n]
    d = np.ascontiguousarray(dist[:, :n])
    with np.errstate(invalid="ignore"):
        hit = cand & (d <= np.asarray(radii, np.float32).reshape(Q, 1))
    bits = d.view(np.uint32).astype(np.uint64)
    rows = []
    for i in range(Q):
        kept = np.flatnonzero(hit[i])[:max_hits].astype(np.uint64)
        rows.append(np.sort((bits[i][kept.astype(np.int64)] << np.uint64(32)) | kept))
    lims = np.zeros(Q + 1, np.uint64)
    np.cumsum([len(r) for r in rows], dtype=np.uint64, out=lims[1:])
    keys = np.concatenate(rows) if rows else np.zeros(0, np.uint64)
    return (lims, keys & np.uint64(0xFFFFFFFF), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), hit.sum(axis=1).astype(np.uint32),
            cand.sum(axis=1).astype(np.uint32))


def rank_radii(dist, rank):
    """each query's radius = its own distance of that rank (clamped to the last)"""
    s = np.sort(dist, axis=1)
    return np.ascontiguousarray(s[:, min(rank, s.shape[1] - 1)])


def first_difference(got, want) -> str:
    """"equal", or the first of lims, ids, distance bits, offered, matched that differs"""
    for name, a, b in zip(("lims", "ids", "dists", "offered", "matched"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        if name == "dists":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape:
            return f"{name}: shape {a.shape} vs {b.shape}"
        bad = np.flatnonzero(a != b)
        if len(bad):
            return f"{name}: {len(bad)} differ, first at {int(bad[0])}: got {a[bad[0]]!r}, want {b[bad[0]]!r}"
    return "equal"
