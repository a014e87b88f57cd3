#!/usr/bin/env python3
"""Multi-vector SpMV against nvec single SpMVs, on one GPU, in one process.

For each matrix (banded 1M x 16, 200^3 7- and 27-point stencils), precision and nvec in 2, 4, 8:
MultiPlan.run (automatic choice) against nvec runs of the automatically chosen Plan on nvec
contiguous vectors. --crossover: on power-law matrices whose slice padding (64 * slots / nnz) is
about 1.2, 2, 4 and 8, the native path (SPMV_HW_KERNEL=slices) against the fallback on the
automatically chosen kernel, which is what sets the automatic choice's padding limit.
--scattered: on the power-law generator at 16 per row (1M, 3M, 10M rows), the one-pass sweep
where the automatic choice takes it against the fallback on the automatically chosen kernel;
with --alt-lib-dir a second build's one-pass sweep beside them.

Protocol (that of graph.cpp time_layout): each form is captured into a graph of --steps runs on
one stream; one untimed replay, then --reps replays each bracketed by events; the two forms of a
pair alternate, round by round. A line reports the median, min and max ms per step over all
rounds, the modelled bytes of the form and the resulting TB/s. One JSON line per form is appended
to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import spmv_hw  # noqa: E402
from ab_variants import stencil  # noqa: E402

KERNEL_NAMES = {0: "tiles", 1: "gold", 2: "sweep", 3: "fpga", 4: "blocked", 5: "slices", 6: "binned"}


class forced_kernel:
    """SPMV_HW_KERNEL set (or unset, for None) while a plan is built."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = os.environ.pop("SPMV_HW_KERNEL", None)
        if self.name:
            os.environ["SPMV_HW_KERNEL"] = self.name

    def __exit__(self, *exc):
        os.environ.pop("SPMV_HW_KERNEL", None)
        if self.old is not None:
            os.environ["SPMV_HW_KERNEL"] = self.old


def capture(fn, steps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # outside the capture: loads what the first run loads
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            fn()
    g.replay()  # untimed
    torch.cuda.synchronize()
    return g


def timed(g, steps, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) / steps for a, b in ev]


def alternate(forms, steps, reps, rounds):
    """forms: {name: fn}. Returns {name: (median, min, max) ms per step}, the forms' replays
    alternating round by round."""
    graphs = {k: capture(fn, steps) for k, fn in forms.items()}
    t = {k: [] for k in forms}
    for _ in range(rounds):
        for k, g in graphs.items():
            t[k] += timed(g, steps, reps)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def slice_stored(rp):
    """64 * slots of the slice layout, from row_ptr alone (slices.hip, build_slices)."""
    lens = np.diff(rp.astype(np.int64))
    pad = (-len(lens)) % 64
    return int(np.pad(lens, (0, pad)).reshape(-1, 64).max(axis=1).sum()) * 64


def slice_model_bytes(stored, n, m, vbytes, fmt, nvec):
    """stored entries * (V + OB) + 4 per row + nvec * (x + y)."""
    ob = 1 if fmt & 8 else 2 if fmt & 1 else 4
    return stored * (vbytes + ob) + 4 * n + nvec * (n + m) * vbytes


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


_STRUCT = {}


def matrix(lib, name, dtype):
    if name == "banded":
        n = 1_000_000
        rp, col, val = spmv_hw.gen_banded(lib, n, 16)
        return rp, col, val, n
    if _STRUCT.get("name") != name:  # the stencil is built once (fp64 values) for both precisions
        _STRUCT.clear()
        _STRUCT.update(name=name, m=stencil(200 ** 3, 7 if name == "stencil7" else 27, np.float64))
    rp, col, val, n = _STRUCT["m"]
    return rp, col, val.to(torch.float64 if dtype == np.float64 else torch.float32), n


def powerlaw_with_padding(lib, n, nnz, target):
    """max_len of the power-law generator (bisected) whose slice padding is closest to target."""
    lo, hi = nnz // n + 1, 65536
    while lo < hi:
        mid = (lo + hi) // 2
        rp, _ = lib.powerlaw_row_ptr(n, nnz, mid, 4)
        if slice_stored(rp) / nnz < target:
            lo = mid + 1
        else:
            hi = mid
    return lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="banded,stencil7,stencil27")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--nvec", default="2,4,8")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--crossover-rows", type=int, default=500_000)
    ap.add_argument("--paddings", default="1.2,2,4,8")
    ap.add_argument("--scattered", action="store_true",
                    help="power-law matrices, 16 per row: the automatically chosen one-pass sweep against the fallback")
    ap.add_argument("--scattered-rows", default="1000000,3000000,10000000")
    ap.add_argument("--force-native", action="store_true", help="structured matrices: SPMV_HW_KERNEL=slices")
    ap.add_argument("--lib-dir", default=None, help="load libspmv_hw_*.so from here (kernel tuning builds)")
    ap.add_argument("--alt-lib-dir", default=None,
                    help="a second build of the libraries, timed beside the first as path 'native (alt build)'")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_bench.jsonl"))
    a = ap.parse_args()
    assert a.steps >= 8 and a.reps * a.rounds >= 7
    if a.lib_dir:
        spmv_hw.LIBDIR = os.path.abspath(a.lib_dir)
    nvecs = [int(v) for v in a.nvec.split(",")]
    def precision(tag):
        dtype = np.float64 if tag == "f64" else np.float32
        return (dtype, torch.float64 if tag == "f64" else torch.float32, np.dtype(dtype).itemsize, spmv_hw.load(dtype),
                {"dtype": tag, "steps": a.steps, "replays": a.reps * a.rounds, "tag": a.tag})

    def alt_library(dtype):
        keep, spmv_hw.LIBDIR = spmv_hw.LIBDIR, os.path.abspath(a.alt_lib_dir)
        try:
            return spmv_hw.Lib(dtype, False)
        finally:
            spmv_hw.LIBDIR = keep

    # --scattered: what decides the automatic choice of the one-pass sweep (multi.cpp,
    # multi_sweep_min_rows). Native: the automatic choice, where it takes the one-pass
    # sweep. Fallback: the kernel the automatic Plan takes for the matrix, named in SPMV_HW_KERNEL so
    # that the handle is the fallback whatever the automatic choice of this build is.
    for tag in (a.dtypes.split(",") if a.scattered else []):
        dtype, td, vb, lib, base = precision(tag)
        alt = alt_library(dtype) if a.alt_lib_dir else None
        for n in [int(v) for v in a.scattered_rows.split(",")]:
            nnz = 16 * n
            rp, col, val, _ = spmv_hw.gen_powerlaw(lib, n, n, nnz, seed=4)
            with forced_kernel(None):
                plan = spmv_hw.Plan.from_device(lib, rp, col, val, n)
            auto = KERNEL_NAMES[plan.stats()["kernel"]]
            plan.destroy()
            for nvec in nvecs:
                with forced_kernel(None):
                    nat = spmv_hw.MultiPlan.from_device(lib, rp, col, val, n, nvec)
                with forced_kernel(auto):
                    fb = spmv_hw.MultiPlan.from_device(lib, rp, col, val, n, nvec)
                nst, fst = nat.stats(), fb.stats()
                assert fst["native"] == 0
                chosen = nst["native"] == 1 and nst["kernel"] == 2 and bool(nst["format"] & 8192)
                X = torch.rand((n, nvec), dtype=td, device="cuda")
                Y = torch.empty((n, nvec), dtype=td, device="cuda")
                forms = {"fallback": lambda: fb.run(X, Y)}
                if chosen:  # (the automatic choice declined: the line of the fallback alone)
                    forms["native"] = lambda: nat.run(X, Y)
                if alt:
                    with forced_kernel(None):
                        nat_alt = spmv_hw.MultiPlan.from_device(alt, rp, col, val, n, nvec)
                    if nat_alt.stats()["native"] == 1:
                        forms["native (alt build)"] = lambda: nat_alt.run(X, Y)
                res = alternate(forms, a.steps, a.reps, a.rounds)
                # native: 14 (fp32: 10) bytes per entry and nvec * (x + y); fallback: the CSR's compulsory bytes
                byts = {"native": nnz * (6 + vb) + nvec * 2 * n * vb, "fallback": fst["algorithmic_bytes"]}
                byts["native (alt build)"] = byts["native"]
                handles = {"native": nat, "fallback": fb, "native (alt build)": nat_alt if alt else None}
                for path in ("native", "fallback", "native (alt build)"):
                    if path not in res:
                        continue
                    med, lo, hi = res[path]
                    st, sweep = handles[path].stats(), path != "fallback"
                    emit(a.out, dict(base, matrix="powerlaw 16 per row", rows=n, nnz=nnz, nvec=nvec, path=path,
                                     kernel=KERNEL_NAMES[st["kernel"]],
                                     panels=int(handles[path].plan_stats()["nr_tiles"]) if sweep else None,
                                     bytes_model="sweep entries" if sweep else "csr", ms=round(med, 5),
                                     ms_min=round(lo, 5), ms_max=round(hi, 5), ms_per_vector=round(med / nvec, 5),
                                     bytes=int(byts[path]), tbps=round(byts[path] / med / 1e9, 4)))
                nat.destroy()
                fb.destroy()
                if alt:
                    nat_alt.destroy()
                del X, Y
            del rp, col, val
            torch.cuda.empty_cache()
    for name in ([] if a.crossover or a.scattered else a.matrices.split(",")):
        for tag in a.dtypes.split(","):
            dtype, td, vb, lib, base = precision(tag)
            alt = alt_library(dtype) if a.alt_lib_dir else None
            rp, col, val, n = matrix(lib, name, dtype)
            stored = slice_stored(rp.cpu().numpy().view(np.uint32))
            nnz = int(rp[-1].item())
            with forced_kernel(None):
                plan = spmv_hw.Plan.from_device(lib, rp, col, val, n)
            pst = plan.stats()
            for nvec in nvecs:
                with forced_kernel("slices" if a.force_native else None):
                    mp = spmv_hw.MultiPlan.from_device(lib, rp, col, val, n, nvec)
                mst = mp.stats()
                X = torch.rand((n, nvec), dtype=td, device="cuda")
                Y = torch.empty((n, nvec), dtype=td, device="cuda")
                xs = [X[:, j].contiguous() for j in range(nvec)]
                ys = [torch.empty(n, dtype=td, device="cuda") for _ in range(nvec)]

                def singles():
                    for j in range(nvec):
                        plan.run(xs[j], ys[j])

                forms = {"single": singles, "multi": lambda: mp.run(X, Y)}
                if alt:
                    with forced_kernel("slices" if a.force_native else None):
                        mp_alt = spmv_hw.MultiPlan.from_device(alt, rp, col, val, n, nvec)
                    forms["alt"] = lambda: mp_alt.run(X, Y)
                res = alternate(forms, a.steps, a.reps, a.rounds)
                single_bytes = nvec * (slice_model_bytes(stored, n, n, vb, pst["format"], 1) if pst["kernel"] == 5
                                       else pst["algorithmic_bytes"])
                multi_bytes = (slice_model_bytes(stored, n, n, vb, mst["format"], nvec) if mst["native"]
                               else mst["algorithmic_bytes"])
                label = {"single": f"{nvec} x single", "multi": "native" if mst["native"] else "fallback",
                         "alt": "native (alt build)"}
                # bytes: the slice layout's stream for slice plans, else the CSR's compulsory bytes
                model = {"single": "slices" if pst["kernel"] == 5 else "csr", "multi": "slices" if mst["native"] else "csr"}
                model["alt"] = model["multi"]
                for path, byt, kern in (("single", single_bytes, pst["kernel"]), ("multi", multi_bytes, mst["kernel"]),
                                        ("alt", multi_bytes, mst["kernel"])):
                    if path not in res:
                        continue
                    med, lo, hi = res[path]
                    emit(a.out, dict(base, matrix=name, rows=n, nnz=nnz, padding=round(stored / nnz, 4), nvec=nvec,
                                     path=label[path], kernel=KERNEL_NAMES[kern], bytes_model=model[path], ms=round(med, 5),
                                     ms_min=round(lo, 5), ms_max=round(hi, 5), ms_per_vector=round(med / nvec, 5),
                                     bytes=int(byt), tbps=round(byt / med / 1e9, 4)))
                mp.destroy()
                if alt:
                    mp_alt.destroy()
                del X, Y, xs, ys
            plan.destroy()
            del rp, col, val
            torch.cuda.empty_cache()
    for tag in (a.dtypes.split(",") if a.crossover else []):
        dtype, td, vb, lib, base = precision(tag)
        n = a.crossover_rows
        nnz = 16 * n
        for target in [float(v) for v in a.paddings.split(",")]:
            max_len = powerlaw_with_padding(lib, n, nnz, target)
            rp, col, val, _ = spmv_hw.gen_powerlaw(lib, n, n, nnz, seed=4, max_len=max_len)
            stored = slice_stored(rp.cpu().numpy().view(np.uint32))
            with forced_kernel(None):
                plan = spmv_hw.Plan.from_device(lib, rp, col, val, n)
            auto = KERNEL_NAMES[plan.stats()["kernel"]]
            plan.destroy()
            for nvec in nvecs:
                with forced_kernel("slices"):
                    nat = spmv_hw.MultiPlan.from_device(lib, rp, col, val, n, nvec)
                with forced_kernel(auto):
                    fb = spmv_hw.MultiPlan.from_device(lib, rp, col, val, n, nvec)
                nst, fst = nat.stats(), fb.stats()
                assert nst["native"] == 1 and fst["native"] == 0
                X = torch.rand((n, nvec), dtype=td, device="cuda")
                Y = torch.empty((n, nvec), dtype=td, device="cuda")
                res = alternate({"native": lambda: nat.run(X, Y), "fallback": lambda: fb.run(X, Y)}, a.steps, a.reps,
                                a.rounds)
                byts = {"native": slice_model_bytes(stored, n, n, vb, nst["format"], nvec),
                        "fallback": fst["algorithmic_bytes"]}
                for path, st in (("native", nst), ("fallback", fst)):
                    med, lo, hi = res[path]
                    emit(a.out, dict(base, matrix=f"powerlaw max_len={max_len}", rows=n, nnz=nnz,
                                     padding=round(stored / nnz, 4), nvec=nvec, path=path,
                                     kernel=KERNEL_NAMES[st["kernel"]],
                                     bytes_model="slices" if path == "native" else "csr", ms=round(med, 5), ms_min=round(lo, 5),
                                     ms_max=round(hi, 5), ms_per_vector=round(med / nvec, 5), bytes=int(byts[path]),
                                     tbps=round(byts[path] / med / 1e9, 4)))
                nat.destroy()
                fb.destroy()
                del X, Y
            del rp, col, val
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
