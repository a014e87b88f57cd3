#!/usr/bin/env python3
"""CGLS for least squares, min ||A x - b||, on a rectangular A — the use the transposed plans are
for: one plan multiplies by A (op N), one by A^T (op T, built on the GPU by the device CSR
transpose), and every iteration is one run of each plus a few vector updates, all on the GPU.
The iteration can be captured once in a CUDA/HIP graph and replayed, as in examples/cg.py.

    python examples/cgls.py [--rows 200000] [--cols 50000] [--tol 1e-10] [--graph]

Matrix: `per_row` seeded random entries per row plus a unit entry at (i, i mod cols), which gives
A full column rank. Stops when ||A^T r|| / ||A^T b|| <= tol (r = b - A x), looked at every
`check_every` iterations, since reading the norm is the one host round trip.
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


def make_matrix(n: int, m: int, per_row: int = 8, seed: int = 1):
    """CSR (row_ptr, col, val) of an n x m matrix: per_row random entries in U(-1, 1) per row and
    a unit entry at (i, i mod m); columns sorted inside a row (a column may repeat: CSR allows it)."""
    rng = np.random.default_rng(seed)
    cols = np.concatenate([rng.integers(0, m, (n, per_row)), (np.arange(n) % m)[:, None]], axis=1)
    vals = np.concatenate([rng.uniform(-1, 1, (n, per_row)), np.ones((n, 1))], axis=1)
    order = np.argsort(cols, axis=1, kind="stable")
    cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
    rp = np.arange(n + 1, dtype=np.int64) * (per_row + 1)
    return rp.astype(np.uint32), cols.ravel().astype(np.uint32), vals.ravel()


def cgls(plan_n, plan_t, b, n_cols: int, tol: float = 1e-10, max_iters: int = 500, use_graph: bool = False,
         check_every: int = 5):
    """(x, iterations, ||A^T r|| / ||A^T b||). plan_n: y = A x, plan_t: y = A^T x; b on the GPU."""
    x = torch.zeros(n_cols, dtype=b.dtype, device=b.device)
    r = b.clone()
    s = torch.empty_like(x)
    q = torch.empty_like(b)
    plan_t.run(r, s)
    p = s.clone()
    gamma = torch.dot(s, s)
    norm0 = float(torch.sqrt(gamma))
    if norm0 == 0.0:
        return x, 0, 0.0

    def step():
        plan_n.run(p, q)
        alpha = gamma / torch.dot(q, q)
        x.add_(alpha * p)
        r.sub_(alpha * q)
        plan_t.run(r, s)
        gamma_new = torch.dot(s, s)
        p.mul_(gamma_new / gamma).add_(s)
        gamma.copy_(gamma_new)

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
    rel = float(torch.sqrt(gamma)) / norm0
    while rel > tol and iters < max_iters:
        for _ in range(min(check_every, max_iters - iters)):
            replay()
            iters += 1
        rel = float(torch.sqrt(gamma)) / norm0
    return x, iters, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--cols", type=int, default=50_000)
    ap.add_argument("--per-row", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iters", type=int, default=500)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    lib = spmv_hw.load(np.float64)
    rp, col, val = make_matrix(a.rows, a.cols, a.per_row)
    dev = lambda h: torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).cuda()
    d = (dev(rp), dev(col), dev(val))
    plan_n = spmv_hw.Plan.from_device(lib, *d, a.cols)
    plan_t = spmv_hw.Plan.from_device(lib, *d, a.cols, transpose=True)
    b = spmv_hw.gen_vector(lib, a.rows, seed=6, lo=-1.0, hi=1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, iters, rel = cgls(plan_n, plan_t, b, a.cols, a.tol, a.max_iters, a.graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"A {a.rows}x{a.cols} nnz={int(rp[-1])} iters={iters} graph={a.graph} time={dt * 1e3:.2f} ms "
          f"({dt * 1e6 / max(iters, 1):.1f} us/iter) relative normal residual {rel:.3e} "
          f"kernels N={plan_n.stats()['kernel']} T={plan_t.stats()['kernel']}")
    plan_n.destroy()
    plan_t.destroy()
    return rel


if __name__ == "__main__":
    main()
