"""The device CSR transpose and the op = T plans on the seeded random matrices of
test_gpu_fuzz.py and the tiny cases of test_gpu_fuzz_multi.py: A^T of 300 000 rows that are
almost all empty, of one row (nr_cols = 1), of unsorted rows with duplicate entries (family 7:
the stable order is what the value bytes test), of a single non-empty row.

The reference transpose is np_transpose of test_gpu_transpose.py (plain numpy, stable); the
reference y is oracle.spmv_gold on those arrays, once per column, never another HIP path. Arrays
are compared bit for bit; plans at TOL and TIGHT of test_gpu_parity.py, and bit for bit where
the kernel promises spmv_gold's bits (the gold kernel, fp64 slices, fp32 slices with
SPMV_SLICE_ACC=32) or, for the blocked kernel, oracle.spmv_fpga_order's. x and X (A's rows) are
uniform in [-1, 1) from default_rng(5000 + seed); y and Y start as NaN.

The rotations shift by one every 8 seeds, because the matrix family is seed % 8: a plain
seed % 8 would tie each family to one kernel."""
import functools

import numpy as np
import pytest

import oracle
import spmv_hw
from test_gpu_fuzz_multi import (CASES, DTYPE, NATIVE_NVEC, TAG, bitwise, case_arrays, case_number, check_columns,
                                 fpga_env, gold_columns, make_X, native_by_rule, run_multi, to_dev, upload_csr)
from test_gpu_parity import KERNEL_ID, TIGHT, TOL
from test_gpu_transpose import np_transpose, same_bits

pytestmark = pytest.mark.gpu

PLAN_KERNELS = ["tiles", "sweep", "slices", "slices_acc32", "binned", "blocked", "gold", "auto"]
MULTI_NVEC = [2, 3, 4, 8]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def plan_kernel(number):
    return PLAN_KERNELS[(number + number // 8) % 8]


def host_range_case(case):
    """Every fourth seed, and the tiny cases of three rows or more, also build their plan with
    Plan.from_host over a row range 0 < r0 < r1 < n."""
    number = case_number(case)
    if case[0] == "s":
        return (number + number // 8) % 4 == 0
    return len(case_arrays(case, np.float64)[0]) - 1 >= 3


def multi_rotation(number):
    """(nvec, SPMV_HW_KERNEL=slices forced?): forced on even numbers, so that 2, 4 and 8 go native
    on A^T whatever its padding; nvec changes every second number, so both parities see all four."""
    return MULTI_NVEC[(number // 2 + number // 8) % 4], number % 2 == 0


@functools.lru_cache(maxsize=4)
def reference(case, tag):
    """A, its numpy transpose, X over A's rows and spmv_gold of A^T per column of X: computed once
    per case and precision; nothing writes to these arrays."""
    row_ptr, col, val, m, unsorted = case_arrays(case, DTYPE[tag])
    t = np_transpose(row_ptr, col, val, m)
    X = make_X(len(row_ptr) - 1, DTYPE[tag], case_number(case))
    return row_ptr, col, val, m, unsorted, t, X, gold_columns(*t, X)


def device_transpose(torch, lib, d_rp, d_col, d_val, nr_cols):
    out = spmv_hw.csr_transpose(lib, d_rp, d_col, d_val, nr_cols)
    torch.cuda.synchronize()
    t_rp, t_col, t_val = (t.cpu().numpy() for t in out)
    return (t_rp.view(np.uint32), t_col.view(np.uint32), t_val), out


def row_range(number, n, inner):
    """A random [r0, r1) with 0 < r0; inner: also r1 < n (needs n >= 3). None when n is too small."""
    rng = np.random.default_rng(7000 + number)
    hi = n - 1 if inner else n
    if hi < 2:
        return None
    r0 = int(rng.integers(1, hi))
    return r0, int(rng.integers(r0 + 1, hi + 1))


# ---- 1. the arrays, bit for bit ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_fuzz_transpose_arrays(torch, case, dtype):
    row_ptr, col, val, m, unsorted, t, _, _ = reference(case, TAG[np.dtype(dtype)])
    n = len(row_ptr) - 1
    lib = spmv_hw.load(dtype)
    d_rp, d_col, d_val = upload_csr(torch, lib, row_ptr, col, val)
    got, dev_t = device_transpose(torch, lib, d_rp, d_col, d_val, m)
    same_bits(got, t)
    # rows [r0, r1) as views of the same device arrays: row_ptr starts at a non-zero offset
    r = row_range(case_number(case), n, inner=False) or (n, n)  # one row: the empty range after it
    r0, r1 = r
    b, e = int(row_ptr[r0]), int(row_ptr[r1])
    part, _ = device_transpose(torch, lib, d_rp[r0:r1 + 1], d_col, d_val, m)
    same_bits(part, np_transpose(row_ptr[r0:r1 + 1], col[b:e], val[b:e], m))
    assert part[1].size == 0 or part[1].max() < r1 - r0  # slice-local source rows
    if not unsorted:  # sorted rows of distinct columns: transposing twice returns A
        back, _ = device_transpose(torch, lib, *dev_t, n)
        same_bits(back, (row_ptr, col, val))


# ---- 2. plans of A^T ----
def run_plan(torch, plan, x, rows):
    y = torch.full((max(rows, 1),), float("nan"), dtype=spmv_hw._torch_dtype(plan.lib.dtype), device="cuda")
    plan.run(to_dev(torch, x), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:rows]


def check_vector(t, x, y_ref, y, dtype, bits):
    t_rp, t_col, t_val = t
    assert not np.any(np.isnan(y) & ~np.isnan(y_ref)), "a row was not written"
    err = oracle.scaled_error(t_rp, t_col, t_val, x, y_ref, y)
    assert err <= TOL[np.dtype(dtype)], err
    assert err <= TIGHT[np.dtype(dtype)], err
    if bits:
        bitwise(y.reshape(-1, 1), y_ref.reshape(-1, 1))
    return err


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_fuzz_transposed_plan(torch, monkeypatch, case, dtype):
    tag, number = TAG[np.dtype(dtype)], case_number(case)
    row_ptr, col, val, m, _, t, X, ref = reference(case, tag)
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    kernel = plan_kernel(number)
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    if kernel == "auto":
        monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    else:
        monkeypatch.setenv("SPMV_HW_KERNEL", kernel.split("_")[0])
    if kernel == "slices_acc32":
        monkeypatch.setenv("SPMV_SLICE_ACC", "32")
    vf, block = fpga_env(monkeypatch, number, n)  # A^T has n columns
    lib = spmv_hw.load(dtype)
    plan = spmv_hw.Plan.from_device(lib, *upload_csr(torch, lib, row_ptr, col, val), m, transpose=True)
    st = plan.stats()
    assert plan.op == 1
    assert (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == (m, n, nnz), st
    assert st["nr_nonempty_rows"] == int((np.diff(t[0].astype(np.int64)) > 0).sum())
    if kernel != "auto":
        assert st["kernel"] == KERNEL_ID[kernel.split("_")[0]], st
    x, y_ref = np.ascontiguousarray(X[:, 0]), np.ascontiguousarray(ref[:, 0])
    y = run_plan(torch, plan, x, m)
    plan.destroy()
    if kernel == "blocked":
        bitwise(y.reshape(-1, 1), oracle.spmv_fpga_order(*t, x, n, block, vf).reshape(-1, 1))
    bits = kernel in ("gold", "slices_acc32") or (kernel == "slices" and np.dtype(dtype) == np.float64)
    err = check_vector(t, x, y_ref, y, dtype, bits)
    print(f"fuzz_transpose plan {case} {tag} {kernel} kernel={st['kernel']} err={err:.3e}")


HOST_CASES = [c for c in CASES if host_range_case(c)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", HOST_CASES)
def test_fuzz_transposed_plan_from_host_row_range(torch, monkeypatch, case, dtype):
    """Plan.from_host(transpose=True) over rows 0 < r0 < r1 < n under the gold kernel: bit for bit
    spmv_gold on the numpy transpose of those rows."""
    row_ptr, col, val, m, _, _, X, _ = reference(case, TAG[np.dtype(dtype)])
    n = len(row_ptr) - 1
    r = row_range(case_number(case), n, inner=True)
    if r is None:
        return  # fewer than three rows: no such range
    r0, r1 = r
    assert 0 < r0 < r1 < n
    monkeypatch.setenv("SPMV_HW_KERNEL", "gold")
    b, e = int(row_ptr[r0]), int(row_ptr[r1])
    t = np_transpose(row_ptr[r0:r1 + 1], col[b:e], val[b:e], m)
    x = np.ascontiguousarray(X[r0:r1, 0])
    lib = spmv_hw.load(dtype)
    plan = spmv_hw.Plan.from_host(lib, lib.make_csr_matrix(row_ptr, col, val, m), r0, r1, transpose=True)
    st = plan.stats()
    assert plan.op == 1 and (st["nr_rows"], st["nr_cols"], st["nr_nzeros"], st["kernel"]) == (m, r1 - r0, e - b, 1), st
    y = run_plan(torch, plan, x, m)
    plan.destroy()
    check_vector(t, x, oracle.spmv_gold(*t, x), y, dtype, True)


# ---- 3. several right-hand sides ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_fuzz_transposed_multi(torch, monkeypatch, case, dtype):
    tag, number = TAG[np.dtype(dtype)], case_number(case)
    row_ptr, col, val, m, _, t, X, ref = reference(case, tag)
    n, nnz = len(row_ptr) - 1, int(row_ptr[-1])
    nvec, forced = multi_rotation(number)
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    if forced:
        monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    else:
        monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    lib = spmv_hw.load(dtype)
    Y, st = run_multi(torch, lib, upload_csr(torch, lib, row_ptr, col, val), n, m, nnz, X, nvec, transpose=True)
    assert Y.shape == (m, nvec)
    if forced:
        assert st["kernel"] == 5 and st["native"] == int(nvec in NATIVE_NVEC), st
    else:  # the automatic choice, on A^T's row lengths
        assert st["native"] == int(native_by_rule(t[0], tag, nvec)), st
    # kernel 5 in fp64, native or once per vector: spmv_gold's bits
    bits = np.dtype(dtype) == np.float64 and st["kernel"] == 5
    err = check_columns(*t, X, ref, Y, dtype, bits)
    print(f"fuzz_transpose multi {case} {tag} nvec={nvec} forced={int(forced)} native={st['native']} "
          f"kernel={st['kernel']} err={err:.3e}")
