#!/usr/bin/env python3
"""Records tests/golden/plan_stats_snapshot.json: for both precisions, every golden matrix and
every forced SPMV_HW_KERNEL name, the plan's stats() fields that describe its layout and the
drop-in wrapper's hw_matrix sizes for one unit (or the create's error text).

The snapshot pins what the built library reports *now*; run it on the commit whose numbers
are to be kept (tests/test_gpu_plan_stats_snapshot.py compares against the file and never
rewrites it). Needs the GPU and built libraries:

    python tools/record_plan_stats.py [--out tests/golden/plan_stats_snapshot.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for _p in (os.path.join(ROOT, "spmv-fpga_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KERNELS = ["tiles", "gold", "sweep", "fpga", "blocked", "slices", "binned"]  # by kernel id
STATS_FIELDS = ["kernel", "nr_tiles", "tile_nnz", "device_bytes", "algorithmic_bytes", "blocks", "format",
                "nr_nonempty_rows"]
HW_FIELDS = ["nr_nzeros", "nr_ci", "nr_val"]
DTYPES = [(np.float64, "f64"), (np.float32, "f32")]


def key(tag, name, kernel):
    return f"{tag}/{name}/{kernel}"


def _dev(torch, a, dtype):
    a = np.ascontiguousarray(a if len(a) else np.zeros(1, dtype))
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def entry(torch, lib, kernel, row_ptr, col, val, x, nr_cols):
    """(snapshot entry, y) of one matrix under the caller's environment (ENV of `kernel`): the
    entry is {"stats": {...}, "hw_matrix": {...}}, or {"error": text} (y None) when the create
    fails."""
    import spmv_hw

    assert os.environ.get("SPMV_HW_KERNEL") == kernel and os.environ.get("SPMV_NGPUS") == "1"
    try:
        plan = spmv_hw.Plan.from_device(lib, _dev(torch, row_ptr, np.uint32), _dev(torch, col, np.uint32),
                                        _dev(torch, val, lib.dtype), nr_cols)
    except RuntimeError as e:
        return {"error": str(e)}, None
    n = len(row_ptr) - 1
    y = torch.full((max(n, 1),), float("nan"), dtype=spmv_hw._torch_dtype(lib.dtype), device="cuda")
    plan.run(_dev(torch, x, lib.dtype), y)
    torch.cuda.synchronize()
    st = plan.stats()
    plan.destroy()
    # the wrapper's view of the same plan (a create that failed above would end the process here)
    hw, bm = lib.create_csr_hw_matrix(lib.make_csr_matrix(row_ptr, col, val, nr_cols))
    u = hw[0].contents
    sizes = {f: int(getattr(u, f)[0]) for f in HW_FIELDS}
    lib.delete_csr_hw_matrix(hw)
    lib.free_bitmap(bm)
    return {"stats": {f: int(st[f]) for f in STATS_FIELDS}, "hw_matrix": sizes}, y.cpu().numpy()[:n]


def env_of(kernel):
    """The environment an entry is taken under: the kernel forced, one unit."""
    return {"SPMV_HW_KERNEL": kernel, "SPMV_NGPUS": "1"}


def main():
    import torch

    import oracle
    import spmv_hw

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(GOLDEN, "plan_stats_snapshot.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "recording needs the GPU"
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        manifest = json.load(f)
    snap = {}
    for dtype, tag in DTYPES:
        lib = spmv_hw.load(dtype)
        for name in sorted(manifest):
            _, c, row_ptr, col, val, _ = oracle.read_csr(os.path.join(GOLDEN, manifest[name]["file"]), dtype)
            x = np.load(os.path.join(GOLDEN, f"{name}.x.{tag}.npy"), allow_pickle=False)
            for kernel in KERNELS:
                os.environ.update(env_of(kernel))
                snap[key(tag, name, kernel)], _ = entry(torch, lib, kernel, row_ptr, col, val, x, c)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(snap, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(snap)} entries ({sum('error' in e for e in snap.values())} create errors) -> {args.out}")


if __name__ == "__main__":
    main()
