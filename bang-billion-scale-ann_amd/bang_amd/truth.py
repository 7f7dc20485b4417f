"""Ground truth from the engine itself: python -m bang_amd.truth [--scan-any] [--scan-radix] <index prefix> <query.bin> <K> <out.bin>

Loads the index (graph in HBM; BANG_EXCLUDE_FILE / BANG_LABEL_FILE are read as by every load), runs the exact scan WITHOUT filters (Engine.scan:
every live point, the distance bits the search returns, equal distances in id order) and writes the harness's ground-truth file (formats.write_truthset:
i32 Q, i32 K, ids u32 [Q][K], distances f32 [Q][K]).  K <= 128; an answer shorter than K (fewer live points) is written with its padding, id
0xFFFFFFFF at distance 3.402823E+38.  The vector type is read from <prefix>_disk_metadata.bin.  The ids of BANG_EXCLUDE_FILE are left out of the
truth; a label table is loaded and changes nothing, since the tool applies no filter (filtered truth: compute(..., any=, all=)).
--scan-any sets the engine option scan_any = 1: float vectors of any D, 8-bit vectors with D % 4 == 0, D <= 1024 (MIPS truth: compute(..., scan_any=1,
mips=True) with queries of D - 1 elements).  --scan-radix sets the engine option scan_radix = 1: K up to 4096 (a recall@1000 truth set), K > 128 on the
radix-select kernels, and the layouts of --scan-any.  Without the flags the tool is what it was.
"""
from __future__ import annotations

import sys

import numpy as np

from . import binding, formats


def index_dtype(prefix: str) -> str:
    """the vector type <prefix>_disk_metadata.bin names"""
    code = formats.read_graph_metadata(prefix + formats.GRAPH_META_SUFFIX)["dtype_code"]
    return {v: k for k, v in formats.PREPROCESS_DTYPE_CODE.items()}[code]


def compute(prefix: str, queries: np.ndarray, K: int, dtype: str | None = None, any=None, all=None, mips: bool = False, **options):
    """-> (ids u32 [Q][K], dists f32 [Q][K], matched u32 [Q]); any / all: per-query label filters over BANG_LABEL_FILE's table; mips (with
    scan_any=1): MIPS search parameters, queries of D - 1 elements"""
    dtype = dtype or index_dtype(prefix)
    options.setdefault("graph", binding.GRAPH_DEVICE)
    with binding.Engine(dtype, **options) as e:
        e.load(prefix)
        if mips:
            e.set_searchparams(K, max(K, 10), binding.DIST_MIPS)
        ids, dists, matched = e.scan(queries, K, any, all)
        e.unload()
    return (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.ascontiguousarray(dists.T), matched


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    options = {}
    if "--scan-any" in argv:
        argv.remove("--scan-any")
        options["scan_any"] = 1
    if "--scan-radix" in argv:
        argv.remove("--scan-radix")
        options["scan_radix"] = 1
    if len(argv) != 4:
        print(__doc__.strip().splitlines()[0], file=sys.stderr)
        return 2
    prefix, qpath, K, out = argv[0], argv[1], int(argv[2]), argv[3]
    dtype = index_dtype(prefix)
    q = formats.read_bin(qpath, dtype)
    ids, dists, matched = compute(prefix, q, K, dtype, **options)
    formats.write_truthset(out, ids, dists)
    print(f"{out}: {ids.shape[0]} queries x {K}, {int(matched.min())} .. {int(matched.max())} live points per query")
    return 0


if __name__ == "__main__":
    sys.exit(main())
