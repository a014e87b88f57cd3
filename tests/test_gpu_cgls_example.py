"""examples/cgls.py: CGLS on a rectangular matrix with one N plan and one T plan reaches its own
tolerance, eagerly and with the iteration captured in a graph. The normal-equation residual
||A^T (b - A x)|| / ||A^T b|| is recomputed on the CPU with scipy from the returned x and held to
10 x tol (the margin covers fp64 rounding in the recomputation)."""
import importlib.util
import os

import numpy as np
import pytest

import spmv_hw
from conftest import ROOT

pytestmark = pytest.mark.gpu

N, M, TOL, MAX_ITERS = 2000, 500, 1e-10, 500


def _example():
    spec = importlib.util.spec_from_file_location("cgls_example", os.path.join(ROOT, "examples", "cgls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("graph", [False, True])
def test_cgls_example_reaches_its_tolerance(graph):
    import scipy.sparse as sp
    import torch
    ex = _example()
    rp, col, val = ex.make_matrix(N, M, per_row=8, seed=1)
    assert rp[-1] == 9 * N and np.all(col.reshape(N, 9) == np.sort(col.reshape(N, 9), axis=1))
    assert all((col[rp[i]:rp[i + 1]] == i % M).any() for i in range(0, N, 97))  # the unit entries
    lib = spmv_hw.load(np.float64)
    dev = lambda h: torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).cuda()
    d = (dev(rp), dev(col), dev(val))
    plan_n = spmv_hw.Plan.from_device(lib, *d, M)
    plan_t = spmv_hw.Plan.from_device(lib, *d, M, transpose=True)
    assert (plan_n.op, plan_t.op) == (0, 1)
    b_h = np.random.default_rng(5).uniform(-1, 1, N)
    x, iters, rel = ex.cgls(plan_n, plan_t, dev(b_h), M, tol=TOL, max_iters=MAX_ITERS, use_graph=graph)
    torch.cuda.synchronize()
    plan_n.destroy()
    plan_t.destroy()
    assert rel <= TOL and 0 < iters <= MAX_ITERS, (rel, iters)
    A = sp.csr_matrix((val, col.astype(np.int64), rp.astype(np.int64)), shape=(N, M))
    x_h = x.cpu().numpy()
    res = np.linalg.norm(A.T @ (b_h - A @ x_h)) / np.linalg.norm(A.T @ b_h)
    print(f"graph={graph}: {iters} iterations, example's residual {rel:.3e}, recomputed {res:.3e}")
    assert res <= 10 * TOL, (res, rel, iters)
