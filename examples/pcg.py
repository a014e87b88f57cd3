#!/usr/bin/env python3
"""Preconditioned conjugate gradient on the GPU: the SpMV plan as the operator and two sparse
triangular solves (spmv_hw.TriSolve, include/csr_hw_wrapper.h Part 5) as a symmetric Gauss-Seidel
preconditioner, z = (D + U)^-1 D (D + L)^-1 r. Both handles are built from the same full matrix A:
the LOWER one uses its lower triangle, the UPPER one its upper triangle.

    python examples/pcg.py [--grid 1000] [--tol 1e-8] [--graph]

Matrix: the shifted 2-D 5-point Laplacian of examples/cg.py with the unknowns in red-black order
(the points with i + j even first). In that order no unknown depends on another of its colour, so
each triangle has 2 dependency levels and a solve is two full-width launches. In the natural
row-major order the same triangle has 2 grid - 1 narrow levels (the anti-diagonals), which solve
one after the other: the script prints the stats of both orders. It then runs plain CG and PCG to
the same relative residual and prints iterations and times.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-fpga_amd"))
import torch  # noqa: E402

import spmv_hw  # noqa: E402


def laplacian_2d(g: int, shift: float = 0.1, red_black: bool = True):
    """CSR (row_ptr, col, val, n) of the 5-point Laplacian on a g x g grid plus shift * I, columns
    sorted per row; red_black: the unknowns (i, j) with i + j even come first, each colour in
    row-major order."""
    n = g * g
    idx = np.arange(n, dtype=np.int64)
    i, j = idx // g, idx % g
    if red_black:
        black = (i + j) % 2 == 1
        new = np.empty(n, np.int64)
        new[~black] = np.arange(int((~black).sum()))
        new[black] = int((~black).sum()) + np.arange(int(black.sum()))
    else:
        new = idx
    rows, cols, vals = [], [], []
    for o, ok in ((-g, i > 0), (-1, j > 0), (0, np.ones(n, bool)), (1, j < g - 1), (g, i < g - 1)):
        rows.append(new[idx[ok]])
        cols.append(new[idx[ok] + o])
        vals.append(np.full(int(ok.sum()), 4.0 + shift if o == 0 else -1.0))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp.astype(np.uint32), cols[order].astype(np.uint32), vals[order], n


def sgs_preconditioner(lower, upper, diag):
    """z = (D + U)^-1 D (D + L)^-1 r as a function (r, z): a LOWER solve, a multiply by the
    diagonal, an UPPER solve (in place on z)."""
    def apply(r, z):
        lower.solve(r, z)
        z.mul_(diag)
        upper.solve(z, z)
    return apply


def pcg(plan, b, tol: float = 1e-8, max_iters: int = 5000, use_graph: bool = False, precond=None,
        check_every: int = 5):
    """(x, iterations, ||r|| / ||b|| of the recurrence). precond(r, z) writes z = M^-1 r; None: plain CG."""
    if precond is None:
        def precond(r, z):
            z.copy_(r)
    x = torch.zeros_like(b)
    r = b.clone()
    z = torch.empty_like(b)
    ap = torch.empty_like(b)
    precond(r, z)
    p = z.clone()
    rz = torch.dot(r, z)
    rr = torch.dot(r, r)
    norm0 = float(torch.sqrt(rr))
    if norm0 == 0.0:
        return x, 0, 0.0

    def step():
        plan.run(p, ap)
        alpha = rz / torch.dot(p, ap)
        x.add_(alpha * p)
        r.sub_(alpha * ap)
        precond(r, z)
        rz_new = torch.dot(r, z)
        p.mul_(rz_new / rz).add_(z)
        rz.copy_(rz_new)
        rr.copy_(torch.dot(r, r))

    replay = step
    iters = 0
    if use_graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm up outside the capture (one real iteration)
            step()
        torch.cuda.current_stream().wait_stream(side)
        iters = 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        replay = g.replay
    rel = float(torch.sqrt(rr)) / norm0
    while rel > tol and iters < max_iters:
        for _ in range(min(check_every, max_iters - iters)):
            replay()
            iters += 1
        rel = float(torch.sqrt(rr)) / norm0
    return x, iters, rel


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--shift", type=float, default=0.1)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iters", type=int, default=5000)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args(argv)
    lib = spmv_hw.load(np.float64)
    dev = lambda h: torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).cuda()
    # what the ordering does to the lower triangle's levels
    rp, col, val, n = laplacian_2d(a.grid, a.shift, red_black=False)
    nat = spmv_hw.TriSolve.from_device(lib, dev(rp), dev(col), dev(val), n, lower=True)
    st_nat = nat.stats()
    nat.destroy()
    rp, col, val, n = laplacian_2d(a.grid, a.shift, red_black=True)
    d = (dev(rp), dev(col), dev(val))
    plan = spmv_hw.Plan.from_device(lib, *d, n)
    lower = spmv_hw.TriSolve.from_device(lib, *d, n, lower=True)
    upper = spmv_hw.TriSolve.from_device(lib, *d, n, lower=False)
    st_rb = lower.stats()
    for name, st in (("natural order", st_nat), ("red-black order", st_rb)):
        print(f"lower triangle, {name}: levels={st['nr_levels']} launches={st['nr_launches']} "
              f"chain_levels={st['nr_chain_levels']} max_level_rows={st['max_level_rows']}")
    diag = torch.full((n,), 4.0 + a.shift, dtype=torch.float64, device="cuda")
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    out = {"n": n, "tol": a.tol, "levels_natural": st_nat["nr_levels"], "levels_red_black": st_rb["nr_levels"]}
    for name, pre in (("cg", None), ("pcg", sgs_preconditioner(lower, upper, diag))):
        pcg(plan, b, a.tol, 5, False, pre)  # untimed: first-use costs of the vector ops and kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, iters, rel = pcg(plan, b, a.tol, a.max_iters, a.graph, pre)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ax = torch.empty_like(b)
        plan.run(x, ax)
        res = float(torch.linalg.norm(b - ax) / torch.linalg.norm(b))
        print(f"{name}: n={n} iters={iters} graph={a.graph} time={dt * 1e3:.2f} ms "
              f"({dt * 1e6 / max(iters, 1):.1f} us/iter) relative residual {res:.3e} (recurrence {rel:.3e})")
        out[name] = {"iters": iters, "ms": dt * 1e3, "residual": res}
    for h in (plan, lower, upper):
        h.destroy()
    return out


if __name__ == "__main__":
    main()
