"""Ground truth from the engine itself: python -m bang_amd.truth <index prefix> <query.bin> <K> <out.bin>

Loads the index (graph in HBM; BANG_EXCLUDE_FILE / BANG_LABEL_FILE are read as by every load), runs the exact scan WITHOUT filters (Engine.scan:
every live point, the distance bits the search returns, equal distances in id order) and writes the harness's ground-truth file (formats.write_truthset:
i32 Q, i32 K, ids u32 [Q][K], distances f32 [Q][K]).  K <= 128; an answer shorter than K (fewer live points) is written with its padding, id
0xFFFFFFFF at distance 3.402823E+38.  The vector type is read from <prefix>_disk_metadata.bin.  The ids of BANG_EXCLUDE_FILE are left out of the
truth; a label table is loaded and changes nothing, since the tool applies no filter (filtered truth: compute(..., any=, all=)).
"""
from __future__ import annotations

import sys

import numpy as np

from . import binding, formats


def index_dtype(prefix: str) -> str:
    """the vector type <prefix>_disk_metadata.bin names"""
    code = formats.read_graph_metadata(prefix + formats.GRAPH_META_SUFFIX)["dtype_code"]
    return {v: k for k, v in formats.PREPROCESS_DTYPE_CODE.items()}[code]


def compute(prefix: str, queries: np.ndarray, K: int, dtype: str | None = None, any=None, all=None, **options):
    """-> (ids u32 [Q][K], dists f32 [Q][K], matched u32 [Q]); any / all: per-query label filters over BANG_LABEL_FILE's table"""
    dtype = dtype or index_dtype(prefix)
    options.setdefault("graph", binding.GRAPH_DEVICE)
    with binding.Engine(dtype, **options) as e:
        e.load(prefix)
        ids, dists, matched = e.scan(queries, K, any, all)
        e.unload()
    return (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(dists.T), matched


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 4:
        print(__doc__.strip().splitlines()[0], file=sys.stderr)
        return 2
    prefix, qpath, K, out = argv[0], argv[1], int(argv[2]), argv[3]
    dtype = index_dtype(prefix)
    q = formats.read_bin(qpath, dtype)
    ids, dists, matched = compute(prefix, q, K, dtype)
    formats.write_truthset(out, ids, dists)
    print(f"{out}: {ids.shape[0]} queries x {K}, {int(matched.min())} .. {int(matched.max())} live points per query")
    return 0


if __name__ == "__main__":
    sys.exit(main())
