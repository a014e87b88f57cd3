#!/usr/bin/env python3
"""Cost of the sparse triangular solve, on one GPU, in one process.

Matrices (lower triangles with a dominant diagonal, values -1 off the diagonal for the grids):
  grid2d / grid2d_rb       the 2-D 5-point grid (--grid2d points per side), natural / red-black order
  grid2d_chain             the same grid at 1024 points per side, natural order: every level is narrow, so
                           the whole solve is ONE chain launch (its time per level against a wide launch's
                           in grid2d is what the cut kTrsvChainRows trades)
  stencil7 / stencil7_rb   the 200^3 7-point stencil, natural / red-black order
  random16                 1M rows, 16 entries per row at random columns < i
For each and each precision: create ms (wall clock around the second TriSolve.from_device, the
device idle before and after: host level analysis, layout build, the copies both ways), levels,
launches, one solve eagerly (--reps solves, each between an event pair after a device sync) and by
graph replay (one solve captured, one untimed replay, --reps replays each between an event pair),
and one SpMV of the same triangle through an ordinary plan by graph replay (--steps runs per graph):
the bandwidth yardstick. One JSON line per matrix and precision is appended to --out.

--alt-lib-dirs name=dir,...: other builds of the libraries (kTrsvChainRows or kTrsvLongRow changed in
spmv_host.hpp) beside this tree's: a handle per build on each matrix, one graph-captured solve each,
the builds' replays alternating round by round (--rounds x --reps each), one line per build with
"what": "build_ab".
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import spmv_hw  # noqa: E402
from multi_bench import emit  # noqa: E402


def grid_lower(shape, red_black, td):
    """Lower triangle (diagonal included) of the 2 d + 1 point stencil on a grid of `shape`, built on
    the GPU: -1 off the diagonal, 2 d + 1.125 on it; red_black: the points with an even coordinate
    sum first. Columns sorted per row. Returns (row_ptr, col, val, n) as Plan.from_device takes them."""
    n = int(np.prod(shape))
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    coords, rest = [], idx
    for s in reversed(shape):
        coords.append(rest % s)
        rest = rest // s
    coords.reverse()
    new = idx
    if red_black:
        black = (sum(coords) % 2) == 1
        nred = int((~black).sum())
        new = torch.empty_like(idx)
        new[~black] = torch.arange(nred, dtype=torch.int64, device="cuda")
        new[black] = nred + torch.arange(n - nred, dtype=torch.int64, device="cuda")
    rows, cols = [new], [new]
    stride = 1
    for k in range(len(shape) - 1, -1, -1):
        for sign in (-1, 1):
            ok = (coords[k] > 0) if sign < 0 else (coords[k] < shape[k] - 1)
            r, c = new[idx[ok]], new[idx[ok] + sign * stride]
            low = c < r
            rows.append(r[low])
            cols.append(c[low])
        stride *= shape[k]
    rows, cols = torch.cat(rows), torch.cat(cols)
    key, _ = torch.sort(rows * n + cols)
    rows, cols = key // n, key % n
    rp = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rp[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    val = torch.where(rows == cols, 2.0 * len(shape) + 1.125, -1.0).to(td)
    return rp.to(torch.int32), cols.to(torch.int32), val, n


def random_lower(n, per, td):
    rng = np.random.default_rng(3)
    rows = np.repeat(np.arange(1, n, dtype=np.int64), per)
    cols = (rng.random(rows.size) * rows).astype(np.int64)
    vals = rng.uniform(-1, 1, rows.size)
    diag = 1.0 + np.bincount(rows, np.abs(vals), n)
    a_rows = np.concatenate([rows, np.arange(n)])
    order = np.argsort(a_rows, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(a_rows, minlength=n))])
    t = lambda h: torch.from_numpy(h).cuda()
    return (t(rp.astype(np.int32)), t(np.concatenate([cols, np.arange(n)])[order].astype(np.int32)),
            t(np.concatenate([vals, diag])[order]).to(td), n)


def matrix(name, td, g2):
    if name == "grid2d_chain":
        return grid_lower((1024, 1024), False, td)
    if name.startswith("grid2d"):
        return grid_lower((g2, g2), name.endswith("_rb"), td)
    if name.startswith("stencil7"):
        return grid_lower((200, 200, 200), name.endswith("_rb"), td)
    if name == "random16":
        return random_lower(1_000_000, 16, td)
    raise SystemExit(f"unknown matrix {name}")


def timed_each(fn, reps):
    """ms of each of `reps` calls of fn, each between an event pair after a device sync."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def captured(fn, steps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def stat3(ts, per=1):
    return {"ms": round(float(np.median(ts)) / per, 5), "ms_min": round(min(ts) / per, 5),
            "ms_max": round(max(ts) / per, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="grid2d,grid2d_rb,grid2d_chain,stencil7,stencil7_rb,random16")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--grid2d", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=8, help="SpMV runs per graph")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3, help="--alt-lib-dirs: rounds of --reps replays per build")
    ap.add_argument("--alt-lib-dirs", default="", help="name=dir,...: other builds timed beside this tree's")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trsv_bench.jsonl"))
    a = ap.parse_args()
    for name in a.matrices.split(","):
        for tag in a.dtypes.split(","):
            dtype = np.float64 if tag == "f64" else np.float32
            td = torch.float64 if tag == "f64" else torch.float32
            lib = spmv_hw.load(dtype)
            rp, col, val, n = matrix(name, td, a.grid2d)
            spmv_hw.TriSolve.from_device(lib, rp, col, val, n).destroy()  # first-use costs, untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tri = spmv_hw.TriSolve.from_device(lib, rp, col, val, n)
            torch.cuda.synchronize()
            create_ms = (time.perf_counter() - t0) * 1e3
            st = tri.stats()
            b = torch.rand(n, dtype=td, device="cuda")
            x = torch.empty_like(b)
            tri.solve(b, x)
            eager = timed_each(lambda: tri.solve(b, x), a.reps)
            g = captured(lambda: tri.solve(b, x), 1)
            replay = timed_each(g.replay, a.reps)
            plan = spmv_hw.Plan.from_device(lib, rp, col, val, n)
            y = torch.empty_like(b)
            gp = captured(lambda: plan.run(b, y), a.steps)
            spmv = timed_each(gp.replay, a.reps)
            rec = {"matrix": name, "dtype": tag, "n": n, "nnz": st["nr_nzeros"], "tag": a.tag,
                   "create_ms": round(create_ms, 2), "levels": st["nr_levels"], "launches": st["nr_launches"],
                   "chain_levels": st["nr_chain_levels"], "max_level_rows": st["max_level_rows"],
                   "device_bytes": st["device_bytes"], "solve_eager": stat3(eager), "solve_graph": stat3(replay),
                   "spmv_graph": stat3(spmv, a.steps), "spmv_kernel": plan.stats()["kernel"], "reps": a.reps}
            rec["solve_over_spmv"] = round(rec["solve_graph"]["ms"] / rec["spmv_graph"]["ms"], 2)
            emit(a.out, rec)
            tri.destroy()
            plan.destroy()
            if a.alt_lib_dirs:
                builds = {"this tree": lib}
                for item in a.alt_lib_dirs.split(","):
                    label, path = item.split("=", 1)
                    keep, spmv_hw.LIBDIR = spmv_hw.LIBDIR, os.path.abspath(path)
                    try:
                        builds[label] = spmv_hw.Lib(dtype, False)
                    finally:
                        spmv_hw.LIBDIR = keep
                tris = {k: spmv_hw.TriSolve.from_device(L, rp, col, val, n) for k, L in builds.items()}
                ref = None
                for k, t in tris.items():  # the cuts move levels between launches, never a sum's order
                    t.solve(b, x)
                    torch.cuda.synchronize()
                    ref = x.clone() if ref is None else ref
                    assert torch.equal(x, ref), f"build {k} gives other bits than this tree"
                graphs = {k: captured((lambda t: lambda: t.solve(b, x))(t), 1) for k, t in tris.items()}
                times = {k: [] for k in tris}
                for _ in range(a.rounds):
                    for k, gk in graphs.items():
                        times[k] += timed_each(gk.replay, a.reps)
                for k, t in tris.items():
                    sk = t.stats()
                    emit(a.out, {"what": "build_ab", "build": k, "matrix": name, "dtype": tag, "n": n, "tag": a.tag,
                                 "levels": sk["nr_levels"], "launches": sk["nr_launches"],
                                 "chain_levels": sk["nr_chain_levels"], "solve_graph": stat3(times[k]),
                                 "replays": a.rounds * a.reps,
                                 "vs_this_tree": round(float(np.median(times[k])) / float(np.median(times["this tree"])), 4)})
                    t.destroy()
                del graphs, tris
            del g, gp, rp, col, val, b, x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
