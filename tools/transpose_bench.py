#!/usr/bin/env python3
"""Cost of the transposed product, on one GPU, in one process.

For each matrix (banded 1M x 16, the 200^3 7-point stencil, the power-law 10M x 10M with 160M
non-zeros) and precision:
  - the device CSR transpose alone (spmv_hw.csr_transpose, median of --treps calls, each between
    two events after a device sync);
  - creating the T plan against creating the N plan (wall clock around Plan.from_device, the
    device idle before and after; the N create is the code path without an op);
  - one SpMV of the T plan against one of the N plan, by graph replay: --steps runs captured into
    one graph, one untimed replay, then --reps replays each between an event pair, the two plans
    alternating round by round (the form of graph.cpp time_layout); median, min and max ms per run;
  - the kernel the automatic choice took for A and for A^T, and with --forced, the T plan built
    with each of those kernels forced (SPMV_HW_KERNEL) and timed the same way, which shows whether
    the automatic choice took the fastest kernel for A^T.
One JSON line per measurement is appended to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import spmv_hw  # noqa: E402
from ab_variants import stencil  # noqa: E402
from multi_bench import KERNEL_NAMES, alternate, emit, forced_kernel  # noqa: E402


def matrix(lib, name, dtype):
    """(row_ptr, col, val, rows, cols) on the GPU."""
    if name == "banded":
        n = 1_000_000
        rp, col, val = spmv_hw.gen_banded(lib, n, 16)
        return rp, col, val, n, n
    if name == "stencil7":
        rp, col, val, n = stencil(200 ** 3, 7, dtype)
        return rp, col, val, n, n
    if name == "powerlaw":
        n, z = 10_000_000, 160_000_000
        rp, col, val, _ = spmv_hw.gen_powerlaw(lib, n, n, z, seed=4)
        return rp, col, val, n, n
    raise SystemExit(f"unknown matrix {name}")


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="banded,stencil7,powerlaw")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--treps", type=int, default=3, help="timed calls of the transpose alone")
    ap.add_argument("--forced", default="tiles,sweep,slices,binned",
                    help="kernels to force on the T plan beside the automatic choice ('' for none)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transpose_bench.jsonl"))
    a = ap.parse_args()
    assert a.reps * a.rounds >= 7
    for name in a.matrices.split(","):
        for tag in a.dtypes.split(","):
            dtype = np.float64 if tag == "f64" else np.float32
            td = torch.float64 if tag == "f64" else torch.float32
            lib = spmv_hw.load(dtype)
            rp, col, val, n, m = matrix(lib, name, dtype)
            nnz = int(rp[-1].item())
            base = {"matrix": name, "dtype": tag, "rows": n, "cols": m, "nnz": nnz, "tag": a.tag}

            # 1. the transpose alone
            spmv_hw.csr_transpose(lib, rp, col, val, m)  # loads the code objects
            ts = []
            for _ in range(a.treps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = spmv_hw.csr_transpose(lib, rp, col, val, m)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
                del out
            torch.cuda.empty_cache()
            emit(a.out, dict(base, what="transpose", ms=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3),
                             ms_max=round(max(ts), 3), calls=a.treps,
                             gnnz_per_s=round(nnz / float(np.median(ts)) / 1e6, 3)))

            # 2. plan create, N against T (automatic kernel choice), second create of each
            with forced_kernel(None):
                for transpose in (False, True):  # untimed: first-use costs (code objects, pinned staging)
                    spmv_hw.Plan.from_device(lib, rp, col, val, m, transpose=transpose).destroy()
                plan_n, ms_n = wall_ms(lambda: spmv_hw.Plan.from_device(lib, rp, col, val, m))
                plan_t, ms_t = wall_ms(lambda: spmv_hw.Plan.from_device(lib, rp, col, val, m, transpose=True))
            st_n, st_t = plan_n.stats(), plan_t.stats()
            assert (plan_n.op, plan_t.op) == (0, 1) and st_t["nr_rows"] == m and st_t["nr_cols"] == n
            emit(a.out, dict(base, what="create", n_ms=round(ms_n, 2), t_ms=round(ms_t, 2),
                             t_over_n=round(ms_t / ms_n, 3), n_kernel=KERNEL_NAMES[st_n["kernel"]],
                             t_kernel=KERNEL_NAMES[st_t["kernel"]], n_device_bytes=st_n["device_bytes"],
                             t_device_bytes=st_t["device_bytes"]))

            # 3. one SpMV, N against T (and T with each forced kernel)
            x_n = torch.rand(m, dtype=td, device="cuda")
            y_n = torch.empty(n, dtype=td, device="cuda")
            x_t = torch.rand(n, dtype=td, device="cuda")
            y_t = torch.empty(m, dtype=td, device="cuda")
            forms = {"N auto": lambda: plan_n.run(x_n, y_n), "T auto": lambda: plan_t.run(x_t, y_t)}
            kernels = {"N auto": st_n["kernel"], "T auto": st_t["kernel"]}
            forced = {}
            for k in [k for k in a.forced.split(",") if k]:
                if k == KERNEL_NAMES[st_t["kernel"]]:
                    continue
                try:
                    with forced_kernel(k):
                        forced[k] = spmv_hw.Plan.from_device(lib, rp, col, val, m, transpose=True)
                except RuntimeError as e:  # a layout that cannot hold this matrix: reported, not timed
                    emit(a.out, dict(base, what="spmv", plan=f"T {k}", error=str(e)))
                    continue
                forms[f"T {k}"] = (lambda p: lambda: p.run(x_t, y_t))(forced[k])
                kernels[f"T {k}"] = forced[k].stats()["kernel"]
            res = alternate(forms, a.steps, a.reps, a.rounds)
            for label, (med, lo, hi) in res.items():
                emit(a.out, dict(base, what="spmv", plan=label, kernel=KERNEL_NAMES[kernels[label]], ms=round(med, 5),
                                 ms_min=round(lo, 5), ms_max=round(hi, 5), steps=a.steps, replays=a.reps * a.rounds,
                                 vs_n=round(med / res["N auto"][0], 3)))
            for p in [plan_n, plan_t] + list(forced.values()):
                p.destroy()
            del rp, col, val, x_n, y_n, x_t, y_t, forms, forced
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
