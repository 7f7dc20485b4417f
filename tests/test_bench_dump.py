"""bench.py --dump-outputs: the arrays the timed path returned in its last step, as DIR/<name>.npy (float64 / float32, at most 64 MB in
all -- a fixed sample of the queries past that).  The end-to-end run on the GPU is in test_gpu_bench.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from tools.bench_legs.common import Ctx  # noqa: E402


def _ctx(world=1):
    ctx = Ctx()
    ctx.world, ctx.weak, ctx.force_gather = world, False, False
    return ctx


def _result(Q, k, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 1 << 40, (Q, k), dtype=np.uint64)
    return {"ids": ids, "dists": rng.random((k, Q), dtype=np.float32)}


def test_dump_writes_what_the_caller_received(tmp_path):
    res = _result(1000, 10)
    bench.dump_outputs(str(tmp_path), res, _ctx())
    assert sorted(os.listdir(tmp_path)) == ["dists.npy", "ids.npy"]
    ids, dists = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "dists.npy")
    assert ids.dtype == np.float64 and ids.shape == (1000, 10) and np.array_equal(ids.astype(np.uint64), res["ids"])
    assert dists.dtype == np.float32 and np.array_equal(dists, res["dists"])


def test_dump_of_a_gathered_step_is_the_whole_batch(tmp_path):
    res = _result(500, 10)                       # rank 0's own block ...
    ctx = _ctx(world=2)
    ctx.batch_ids = _result(1000, 10, seed=1)["ids"]  # ... and the batch the all-gather delivered
    bench.dump_outputs(str(tmp_path), res, ctx)
    assert np.array_equal(np.load(tmp_path / "ids.npy").astype(np.uint64), ctx.batch_ids)
    assert np.array_equal(np.load(tmp_path / "dists.npy"), res["dists"])


def test_dump_past_the_cap_is_a_fixed_sample(tmp_path):
    Q, k = 600_000, 10                           # 72 MB of ids + dists
    res = _result(Q, k)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, _ctx())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_CAP_BYTES
    rows = np.load(tmp_path / "a" / "query_rows.npy").astype(np.int64)
    assert rows.size > Q // 2 and (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy").astype(np.uint64), res["ids"][rows])
    assert np.array_equal(np.load(tmp_path / "a" / "dists.npy"), res["dists"][:, rows])
    for f in ("ids.npy", "dists.npy", "query_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
