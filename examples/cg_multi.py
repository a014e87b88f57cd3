#!/usr/bin/env python3
"""Conjugate gradient for several right-hand sides at once: `--nvec` independent CG solves share
one multi-vector SpMV per iteration (spmv_hw.MultiPlan), so the matrix is streamed from HBM once
per iteration instead of once per right-hand side. Every solve keeps its own alpha and beta
(column-wise reductions); with --graph the whole iteration is captured once and replayed, as in
cg.py.

    python examples/cg_multi.py [--grid 1000] [--iters 200] [--nvec 4] [--graph]

Matrix: cg.py's 2-D 5-point Laplacian plus a diagonal shift (SPD). B has nvec different columns.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-fpga_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch  # noqa: E402

import spmv_hw  # noqa: E402
from cg import laplacian_2d  # noqa: E402


def cg_multi(mp, B, iters: int, use_graph: bool):
    """Unpreconditioned CG on every column of B, fixed iteration count, all state on the GPU."""
    X = torch.zeros_like(B)
    R = B.clone()
    P = R.clone()
    AP = torch.empty_like(B)
    rr = (R * R).sum(dim=0)  # one scalar per column

    def step():
        mp.run(P, AP)
        alpha = rr / (P * AP).sum(dim=0)
        X.add_(alpha * P)
        R.sub_(alpha * AP)
        rr_new = (R * R).sum(dim=0)
        P.mul_(rr_new / rr).add_(R)
        rr.copy_(rr_new)

    if not use_graph:
        for _ in range(iters):
            step()
        return X
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture (one real iteration)
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(iters - 1):
        g.replay()
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--nvec", type=int, default=4)
    ap.add_argument("--graph", action="store_true")
    a = ap.parse_args()
    lib = spmv_hw.load(np.float64)
    rp, col, val, n = laplacian_2d(a.grid)
    dev = lambda h: torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).cuda()
    mp = spmv_hw.MultiPlan.from_device(lib, dev(rp), dev(col), dev(val), n, a.nvec)
    # nvec different right-hand sides: ones, and smooth waves of growing frequency
    t = torch.linspace(0, 1, n, dtype=torch.float64, device="cuda")
    B = torch.stack([torch.cos(j * np.pi * t) + (1.0 if j == 0 else 0.5) for j in range(a.nvec)], dim=1).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X = cg_multi(mp, B, a.iters, a.graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    AX = torch.empty_like(B)
    mp.run(X, AX)
    res = (torch.linalg.norm(B - AX, dim=0) / torch.linalg.norm(B, dim=0)).cpu().tolist()
    st = mp.stats()
    print(f"n={n} nnz={int(rp[-1])} nvec={a.nvec} iters={a.iters} graph={a.graph} time={dt * 1e3:.2f} ms "
          f"({dt * 1e6 / a.iters:.1f} us/iter) native={st['native']} kernel={st['kernel']}")
    for j, r in enumerate(res):
        print(f"column {j}: relative residual {r:.3e}")
    mp.destroy()
    return res


if __name__ == "__main__":
    main()
