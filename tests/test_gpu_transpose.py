"""Transposed SpMV: the device CSR transpose (spmv_hw.csr_transpose) and the op = T plans.

The reference transpose is plain numpy, independent of the code under test: a stable argsort of
the columns, the source rows and values taken in that order, row_ptr from a bincount. The
reference y is oracle.spmv_gold on those arrays, never another HIP path. Arrays are compared bit
for bit (indices and value bytes); plans at the bounds of tests/test_gpu_parity.py (scaled error
1e-6 / 1e-12 fp64, 1e-4 / 2e-6 fp32), and bitwise where the kernel promises spmv_gold's bits (the
gold kernel, fp64 slices, fp32 slices with SPMV_SLICE_ACC=32). y starts as NaN.
"""
import functools
import os

import numpy as np
import pytest

import oracle
import spmv_hw
from conftest import DTYPES, FIXTURES, GOLDEN, manifest

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-4}
TIGHT = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2e-6}
KERNEL_ID = {"tiles": 0, "gold": 1, "sweep": 2, "blocked": 4, "slices": 5, "binned": 6}
TAG = {np.dtype(d): t for d, t in DTYPES}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def np_transpose(row_ptr, col, val, nr_cols):
    """(t_row_ptr, t_col, t_val) of A^T, stable: plain numpy."""
    rp = np.asarray(row_ptr).astype(np.int64)
    rp = rp - rp[0]
    n = len(rp) - 1
    row_of_entry = np.repeat(np.arange(n, dtype=np.uint32), np.diff(rp))
    order = np.argsort(col, kind="stable")
    t_col = row_of_entry[order]
    t_val = val[order]
    t_rp = np.zeros(nr_cols + 1, np.int64)
    t_rp[1:] = np.cumsum(np.bincount(col.astype(np.int64), minlength=nr_cols))
    return t_rp.astype(np.uint32), t_col.astype(np.uint32), np.ascontiguousarray(t_val)


def device_transpose(torch, lib, row_ptr, col, val, nr_cols):
    out = spmv_hw.csr_transpose(lib, to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val), nr_cols)
    torch.cuda.synchronize()
    t_rp, t_col, t_val = (t.cpu().numpy() for t in out)
    return t_rp.view(np.uint32), t_col.view(np.uint32), t_val


def same_bits(got, ref):
    for g, r, what in zip(got, ref, ("row_ptr", "col_ind", "values")):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            w = g.dtype.itemsize
            diff = np.nonzero((g.view(np.uint8).reshape(-1, w) != r.view(np.uint8).reshape(-1, w)).any(axis=1))[0]
            raise AssertionError(f"{what}: first differing elements {diff[:5]}")


def csr_from_rows(rows, dtype, seed):
    """rows: one integer array of columns per row, kept in the order given."""
    lens = np.array([len(r) for r in rows], np.int64)
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    col = (np.concatenate(rows) if len(rows) and rp[-1] else np.zeros(0)).astype(np.uint32)
    # distinct values: a wrong order inside a transposed row shows in the value bytes
    val = np.random.default_rng(seed).permutation(len(col)).astype(dtype) + dtype(0.25)
    return rp.astype(np.uint32), col, val


KEY_BIT_COLS = [1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 17 + 1]


def _key_bits_case(m, dtype):
    """300 rows of random columns below m, with entries in column 0 and the last two columns."""
    rng = np.random.default_rng(m)
    rows = [rng.integers(0, m, rng.integers(0, 6)) for _ in range(300)]
    ends = np.unique(np.clip([0, m - 2, m - 1], 0, m - 1))
    rows[7] = np.concatenate([rows[7], ends])
    rows[250] = np.concatenate([ends[::-1], rows[250]])
    return csr_from_rows(rows, dtype, m) + (m,)


def _structure_case(name, dtype):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "nnz0":
        return np.zeros(101, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 50
    if name == "rows0":
        return np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 5
    if name == "cols0":
        return np.zeros(4, np.uint32), np.zeros(0, np.uint32), np.zeros(0, dtype), 0
    if name == "hot_column":  # 5000 x 7, column 3 holds every row: one long transposed row
        rows = [np.unique(np.concatenate([[3], rng.integers(0, 7, rng.integers(0, 3))])) for _ in range(5000)]
        return csr_from_rows(rows, dtype, 1) + (7,)
    if name == "duplicates_unsorted":  # duplicate (r, c) entries, columns in any order inside a row
        rows = [rng.integers(0, 40, rng.integers(0, 30)) for _ in range(700)]
        rows[3] = np.array([5, 5, 2, 5, 39, 0, 2])
        return csr_from_rows(rows, dtype, 2) + (40,)
    if name == "empty_rows_and_columns":  # leading, interior and trailing empty rows and columns
        n, m = 900, 600
        rows = [np.zeros(0, np.int64)] * n
        for r in list(range(100, 400)) + list(range(450, 800)):
            rows[r] = np.sort(rng.choice(np.r_[50:200, 260:540], rng.integers(1, 9), replace=False))
        return csr_from_rows(rows, dtype, 3) + (m,)
    raise KeyError(name)


STRUCTURE_CASES = ["nnz0", "rows0", "cols0", "hot_column", "duplicates_unsorted", "empty_rows_and_columns"]


@functools.lru_cache(maxsize=None)
def fixture_case(name, tag):
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    n, c, row_ptr, col, val, _ = oracle.read_csr(os.path.join(GOLDEN, manifest()[name]["file"]), dtype)
    return row_ptr, col, val, c


@functools.lru_cache(maxsize=None)
def powerlaw_case(tag):
    """The rectangular power-law matrix, 20000 x 7000 with 320k non-zeros (many workgroups), from
    the library's generator; its numpy transpose is computed once per precision."""
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    lib = spmv_hw.load(dtype)
    rp, col, val, _ = spmv_hw.gen_powerlaw(lib, 20_000, 7_000, 320_000, seed=4)
    row_ptr, col, val = rp.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32), val.cpu().numpy()
    assert row_ptr[-1] == 320_000
    return row_ptr, col, val, 7_000


def case_arrays(case, dtype):
    tag = TAG[np.dtype(dtype)]
    if case in FIXTURES:
        return fixture_case(case, tag)
    if case == "powerlaw":
        return powerlaw_case(tag)
    if case.startswith("cols_"):
        return _key_bits_case(int(case[5:]), dtype)
    return _structure_case(case, dtype)


@functools.lru_cache(maxsize=None)
def reference(case, tag):
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    row_ptr, col, val, m = case_arrays(case, dtype)
    return np_transpose(row_ptr, col, val, m)


ARRAY_CASES = FIXTURES + STRUCTURE_CASES + [f"cols_{m}" for m in KEY_BIT_COLS] + ["powerlaw"]


# ---- 1. the arrays, bit for bit ----
@pytest.mark.parametrize("case", ARRAY_CASES)
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_csr_transpose_equals_numpy_bit_for_bit(torch, case, dtype, tag):
    row_ptr, col, val, m = case_arrays(case, dtype)
    ref = reference(case, tag)
    lib = spmv_hw.load(dtype)
    got = device_transpose(torch, lib, row_ptr, col, val, m)
    same_bits(got, ref)
    assert got[0][0] == 0 and got[0][-1] == len(col)
    if len(col):  # stable: the source rows of one transposed row do not decrease
        inner = np.ones(len(col), bool)
        inner[ref[0][:-1][ref[0][:-1] < len(col)]] = False
        assert np.all(np.diff(got[1].astype(np.int64))[inner[1:]] >= 0)
    again = device_transpose(torch, lib, row_ptr, col, val, m)  # deterministic
    same_bits(again, got)


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_row_ptr_at_an_offset_device_slice(torch, dtype, tag):
    """Rows [r0, r1) of a larger CSR given as views of its device arrays: row_ptr starts at a
    non-zero offset, the transposed source rows are slice-local and the output row_ptr starts at 0."""
    row_ptr, col, val, m = powerlaw_case(tag)
    lib = spmv_hw.load(dtype)
    d_rp, d_col, d_val = to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val)
    for r0, r1 in ((1, 20_000), (7_001, 13_337), (19_999, 20_000), (500, 500)):
        b, e = int(row_ptr[r0]), int(row_ptr[r1])
        assert r0 == r1 or b > 0
        out = spmv_hw.csr_transpose(lib, d_rp[r0:r1 + 1], d_col, d_val, m)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in out]
        got = (got[0].view(np.uint32), got[1].view(np.uint32), got[2])
        same_bits(got, np_transpose(row_ptr[r0:r1 + 1], col[b:e], val[b:e], m))
        assert got[1].size == 0 or got[1].max() < r1 - r0


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_round_trip_returns_a(torch, dtype, tag):
    """Sorted columns and no duplicates: transposing twice gives A back, bit for bit."""
    lib = spmv_hw.load(dtype)
    for case in ("powerlaw", "empty_rows_and_columns", "small", "wide"):
        row_ptr, col, val, m = case_arrays(case, dtype)
        n = len(row_ptr) - 1
        t = spmv_hw.csr_transpose(lib, to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val), m)
        tt = spmv_hw.csr_transpose(lib, t[0], t[1], t[2], n)
        torch.cuda.synchronize()
        got = [a.cpu().numpy() for a in tt]
        same_bits((got[0].view(np.uint32), got[1].view(np.uint32), got[2]), (row_ptr, col, val))


# ---- 2. plans of A^T ----
PLAN_KERNELS = ["tiles", "sweep", "slices", "slices_acc32", "binned", "blocked", "gold", "auto"]


@pytest.fixture(params=PLAN_KERNELS)
def kernel(request, monkeypatch):
    """SPMV_HW_KERNEL forced to each kernel in turn, and once unset ("auto": the automatic choice
    on A^T); "slices_acc32" is the slice kernel with SPMV_SLICE_ACC=32 (fp32 sums in fp32)."""
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    if request.param == "auto":
        monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    else:
        monkeypatch.setenv("SPMV_HW_KERNEL", request.param.split("_")[0])
    if request.param == "slices_acc32":
        monkeypatch.setenv("SPMV_SLICE_ACC", "32")
    return request.param


def bitwise_kernel(kernel, dtype):
    return kernel in ("gold", "slices_acc32") or (kernel == "slices" and np.dtype(dtype) == np.float64)


@functools.lru_cache(maxsize=None)
def plan_reference(case, tag):
    """x (A's rows), the oracle's y = A^T x on the numpy transpose, and the same for A itself."""
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    row_ptr, col, val, m = case_arrays(case, dtype)
    n = len(row_ptr) - 1
    rng = np.random.default_rng(sum(map(ord, case)))
    x_t = rng.uniform(0, 1, n).astype(dtype)
    x_n = rng.uniform(0, 1, m).astype(dtype)
    t_rp, t_col, t_val = reference(case, tag)
    return x_t, oracle.spmv_gold(t_rp, t_col, t_val, x_t), x_n, oracle.spmv_gold(row_ptr, col, val, x_n)


def run_plan(torch, plan, x, rows):
    y = torch.full((max(rows, 1),), float("nan"), dtype=spmv_hw._torch_dtype(plan.lib.dtype), device="cuda")
    plan.run(to_dev(torch, x if len(x) else np.zeros(1, plan.lib.dtype)), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:rows]


def check(t_rp, t_col, t_val, x, y_ref, y, dtype, bitwise):
    assert not np.any(np.isnan(y) & ~np.isnan(y_ref)), "a row was not written"
    err = oracle.scaled_error(t_rp, t_col, t_val, x, y_ref, y)
    assert err <= TOL[np.dtype(dtype)], err
    assert err <= TIGHT[np.dtype(dtype)], err
    if bitwise:
        assert np.array_equal(y.view(np.uint8), y_ref.view(np.uint8)), "not spmv_gold's bits"


@pytest.mark.parametrize("case", FIXTURES + ["powerlaw"])
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_transposed_plan_matches_oracle(torch, kernel, case, dtype, tag):
    row_ptr, col, val, m = case_arrays(case, dtype)
    n = len(row_ptr) - 1
    t_rp, t_col, t_val = reference(case, tag)
    x_t, y_t, x_n, y_n = plan_reference(case, tag)
    lib = spmv_hw.load(dtype)
    dev = [to_dev(torch, a) for a in (row_ptr, col, val)]
    plan = spmv_hw.Plan.from_device(lib, *dev, m, transpose=True)
    st = plan.stats()
    assert plan.op == 1
    assert (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == (m, n, len(col))
    assert st["nr_nonempty_rows"] == int((np.diff(t_rp.astype(np.int64)) > 0).sum())
    if kernel != "auto":
        assert st["kernel"] == KERNEL_ID[kernel.split("_")[0]]
    check(t_rp, t_col, t_val, x_t, y_t, run_plan(torch, plan, x_t, m), dtype, bitwise_kernel(kernel, dtype))
    plan.destroy()
    # an N plan of the same matrix is what it was: op 0, A's shape, its own oracle y
    plan = spmv_hw.Plan.from_device(lib, *dev, m)
    st = plan.stats()
    assert plan.op == 0 and (st["nr_rows"], st["nr_cols"]) == (n, m)
    check(row_ptr, col, val, x_n, y_n, run_plan(torch, plan, x_n, n), dtype, bitwise_kernel(kernel, dtype))
    plan.destroy()


@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_transposed_plan_from_host_row_range(torch, monkeypatch, dtype, tag):
    """from_host with 0 < row_begin < row_end < n: the slice is uploaded, rebased and transposed;
    the gold kernel's y is bitwise spmv_gold on the numpy transpose of those rows."""
    monkeypatch.setenv("SPMV_HW_KERNEL", "gold")
    row_ptr, col, val, m = powerlaw_case(tag)
    lib = spmv_hw.load(dtype)
    mat = lib.make_csr_matrix(row_ptr, col, val, m)
    for r0, r1 in ((3, 19_990), (9_000, 9_001)):
        b, e = int(row_ptr[r0]), int(row_ptr[r1])
        t_rp, t_col, t_val = np_transpose(row_ptr[r0:r1 + 1], col[b:e], val[b:e], m)
        x = np.random.default_rng(r0).uniform(0, 1, r1 - r0).astype(dtype)
        plan = spmv_hw.Plan.from_host(lib, mat, r0, r1, transpose=True)
        st = plan.stats()
        assert plan.op == 1 and (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == (m, r1 - r0, e - b)
        check(t_rp, t_col, t_val, x, oracle.spmv_gold(t_rp, t_col, t_val, x), run_plan(torch, plan, x, m), dtype, True)
        plan.destroy()


# ---- 3. graphs ----
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_transposed_plan_in_graphs(torch, dtype, tag):
    """The T plan captured into a torch graph and replayed twice, and through run_graph(iters=3)."""
    row_ptr, col, val, m = powerlaw_case(tag)
    t_rp, t_col, t_val = reference("powerlaw", tag)
    x_t, y_t, _, _ = plan_reference("powerlaw", tag)
    lib = spmv_hw.load(dtype)
    plan = spmv_hw.Plan.from_device(lib, to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val), m,
                                    transpose=True)
    x = to_dev(torch, x_t)
    y = torch.full((m,), float("nan"), dtype=x.dtype, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        plan.run(x, y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(x, y)
    for _ in range(2):
        y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        check(t_rp, t_col, t_val, x_t, y_t, y.cpu().numpy(), dtype, False)
    del g
    y2 = torch.full((m,), float("nan"), dtype=x.dtype, device="cuda")
    plan.run_graph(x, y2, iters=3)
    torch.cuda.synchronize()
    check(t_rp, t_col, t_val, x_t, y_t, y2.cpu().numpy(), dtype, False)
    plan.destroy()


# ---- 4. several right-hand sides ----
@functools.lru_cache(maxsize=None)
def banded_case(tag):
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    lib = spmv_hw.load(dtype)
    n = 100_000
    rp, col, val = spmv_hw.gen_banded(lib, n, 16, seed=2)
    row_ptr, col, val = rp.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32), val.cpu().numpy()
    t = np_transpose(row_ptr, col, val, n)
    X = np.random.default_rng(8).uniform(0, 1, size=(n, 8)).astype(dtype)
    ref = np.stack([oracle.spmv_gold(*t, np.ascontiguousarray(X[:, j])) for j in range(8)], axis=1)
    return row_ptr, col, val, n, t, X, ref


@pytest.mark.parametrize("dtype,tag", DTYPES)
@pytest.mark.parametrize("nvec", [2, 3, 4, 8])
def test_transposed_multi_vector(torch, monkeypatch, dtype, tag, nvec):
    """MultiPlan(transpose=True) on the banded 100k x 16 matrix: nvec 2, 4 and 8 take the native
    one-pass kernel (bitwise spmv_gold in fp64), nvec 3 the per-vector fallback."""
    monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    row_ptr, col, val, n, t, X, ref = banded_case(tag)
    lib = spmv_hw.load(dtype)
    mp = spmv_hw.MultiPlan.from_device(lib, to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val), n, nvec,
                                       transpose=True)
    st = mp.stats()
    assert mp.op == 1 and st["nvec"] == nvec and st["native"] == (0 if nvec == 3 else 1)
    assert (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == (n, n, len(col))
    Xd = to_dev(torch, X[:, :nvec])
    Y = torch.full((n, nvec), float("nan"), dtype=Xd.dtype, device="cuda")
    mp.run(Xd, Y)
    torch.cuda.synchronize()
    mp.destroy()
    Yh = Y.cpu().numpy()
    for j in range(nvec):
        check(*t, np.ascontiguousarray(X[:, j]), np.ascontiguousarray(ref[:, j]), np.ascontiguousarray(Yh[:, j]), dtype,
              nvec != 3 and np.dtype(dtype) == np.float64)


def test_transposed_multi_shape_checks_use_the_transposed_dimensions(torch):
    """A rectangular A (20000 x 7000): X is (20000, nvec), Y is (7000, nvec); A's own shapes are refused."""
    row_ptr, col, val, m = powerlaw_case("f64")
    n = len(row_ptr) - 1
    lib = spmv_hw.load(np.float64)
    mat = lib.make_csr_matrix(row_ptr, col, val, m)
    for mp in (spmv_hw.MultiPlan.from_device(lib, to_dev(torch, row_ptr), to_dev(torch, col), to_dev(torch, val), m, 2,
                                             transpose=True),
               spmv_hw.MultiPlan.from_host(lib, mat, 0, n, 2, transpose=True)):
        assert (mp.nr_rows, mp.nr_cols, mp.op) == (m, n, 1)
        X = torch.rand((n, 2), dtype=torch.float64, device="cuda")
        Y = torch.full((m, 2), float("nan"), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            mp.run(Y, X)
        mp.run(X, Y)
        torch.cuda.synchronize()
        t = reference("powerlaw", "f64")
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        for j in range(2):
            xj = np.ascontiguousarray(Xh[:, j])
            check(*t, xj, oracle.spmv_gold(*t, xj), np.ascontiguousarray(Yh[:, j]), np.float64, False)
        mp.destroy()


# ---- 5. refusals ----
def test_out_of_range_column_is_refused(torch):
    lib = spmv_hw.load(np.float64)
    rp, col, val = (to_dev(torch, a) for a in (np.array([0, 2, 3], np.uint32), np.array([0, 5, 1], np.uint32),
                                               np.ones(3)))
    with pytest.raises(RuntimeError, match="out of range"):
        spmv_hw.csr_transpose(lib, rp, col, val, 5)
    with pytest.raises(RuntimeError, match="out of range"):
        spmv_hw.Plan.from_device(lib, rp, col, val, 5, transpose=True)
    with pytest.raises(RuntimeError, match="out of range"):
        spmv_hw.MultiPlan.from_device(lib, rp, col, val, 5, 2, transpose=True)
    torch.cuda.synchronize()


def test_more_than_2_31_minus_1_nonzeros_are_refused_before_the_entries_are_touched(torch):
    """row_ptr = [0, 2^31] with one-element col and val tensors: the refusal names the limit and
    comes before anything reads the entry arrays (which hold one element)."""
    lib = spmv_hw.load(np.float64)
    rp = to_dev(torch, np.array([0, 2 ** 31], np.uint32))
    col, val = to_dev(torch, np.zeros(1, np.uint32)), to_dev(torch, np.ones(1))
    with pytest.raises(RuntimeError, match=r"2\^31 - 1"):
        spmv_hw.csr_transpose(lib, rp, col, val, 4)
    with pytest.raises(RuntimeError, match=r"2\^31 - 1"):
        spmv_hw.Plan.from_device(lib, rp, col, val, 4, transpose=True)
    with pytest.raises(RuntimeError, match=r"2\^31 - 1"):
        spmv_hw.MultiPlan.from_device(lib, rp, col, val, 4, 2, transpose=True)
    t_rp = torch.zeros(5, dtype=torch.int32, device="cuda")
    rc = lib.L.spmv_csr_transpose_device(0, 1, 4, 2 ** 31, rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                         t_rp.data_ptr(), None, None, None)
    assert rc != 0 and "2^31 - 1" in lib.L.spmv_hw_last_error().decode()
    torch.cuda.synchronize()  # nothing was enqueued that could fault
