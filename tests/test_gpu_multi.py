"""Multi-vector SpMV (spmv_multi_*, MultiPlan): Y = A X for 1..8 right-hand sides per run.

Every column j of Y is compared with the CPU oracle on column j of X (oracle.spmv_gold), never
with the single-vector HIP path. The native path (one pass over the slice layout, nvec 2 / 4 / 8)
is bit for bit spmv_gold in fp64, and in fp32 with SPMV_SLICE_ACC=32; otherwise the bounds are
those of test_gpu_parity.py (scaled error 1e-6 / 1e-12 fp64, 1e-4 / 2e-6 fp32). Y starts as NaN.
"""
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import spmv_hw
from conftest import DTYPES, FIXTURES, GOLDEN, manifest

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-4}
TIGHT = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2e-6}
KERNEL_ID = {"tiles": 0, "gold": 1, "sweep": 2, "blocked": 4, "slices": 5, "binned": 6}
NATIVE_NVEC = (2, 4, 8)
MAXVEC = 8


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


def make_X(m, dtype, seed):
    """MAXVEC distinct seeded columns in [0, 1); a run with nvec vectors takes the first nvec."""
    return np.random.default_rng(seed).uniform(0, 1, size=(m, MAXVEC)).astype(dtype)


def gold_columns(row_ptr, col, val, X):
    """The oracle's y for every column of X, and the proof that the columns tell a swapped or
    broadcast Y apart: the per-column results differ pairwise (when the matrix has entries)."""
    ref = np.stack([oracle.spmv_gold(row_ptr, col, val, np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])],
                   axis=1)
    if len(col):
        for a in range(X.shape[1]):
            for b in range(a + 1, X.shape[1]):
                assert not np.array_equal(ref[:, a], ref[:, b]), (a, b)
    return ref


def build(torch, lib, row_ptr, col, val, nr_cols, nvec):
    return spmv_hw.MultiPlan.from_device(lib, to_dev(torch, row_ptr),
                                         to_dev(torch, col if len(col) else np.zeros(1, np.uint32)),
                                         to_dev(torch, val if len(val) else np.zeros(1, lib.dtype)), nr_cols, nvec)


def run_multi(torch, lib, row_ptr, col, val, X, nvec):
    """(Y as numpy (n, nvec), stats) of one run on the first nvec columns of X; Y pre-filled NaN."""
    n, m = len(row_ptr) - 1, X.shape[0]
    mp = build(torch, lib, row_ptr, col, val, m, nvec)
    Xd = to_dev(torch, X[:, :nvec])
    Y = torch.full((n, nvec), float("nan"), dtype=Xd.dtype, device="cuda")
    mp.run(Xd, Y)
    torch.cuda.synchronize()
    st = mp.stats()
    mp.destroy()
    assert st["nvec"] == nvec and st["nr_rows"] == n and st["nr_cols"] == m and st["nr_nzeros"] == int(row_ptr[-1])
    return Y.cpu().numpy(), st


def bitwise(Y, ref):
    assert Y.dtype == ref.dtype and Y.shape == ref.shape
    same = Y.view(np.uint8).reshape(Y.shape[0], -1) == np.ascontiguousarray(ref).view(np.uint8).reshape(Y.shape[0], -1)
    assert same.all(), f"first differing rows {np.nonzero(~same.all(axis=1))[0][:5]}"


def check(row_ptr, col, val, X, ref, Y, dtype):
    for j in range(Y.shape[1]):
        y, r, x = Y[:, j], ref[:, j], np.ascontiguousarray(X[:, j])
        assert not np.any(np.isnan(y) & ~np.isnan(r)), f"column {j}: a row was not written"
        err = oracle.scaled_error(row_ptr, col, val, x, r, y)
        assert err <= TOL[np.dtype(dtype)], (j, err)
        assert err <= TIGHT[np.dtype(dtype)], (j, err)


# ---- 1. native path on the golden fixtures ----
@functools.lru_cache(maxsize=None)
def fixture_case(name, tag):
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    _, c, row_ptr, col, val, _ = oracle.read_csr(os.path.join(GOLDEN, manifest()[name]["file"]), dtype)
    X = make_X(c, dtype, seed=sum(map(ord, name)))
    return row_ptr, col, val, X, gold_columns(row_ptr, col, val, X)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("dtype,tag", DTYPES)
@pytest.mark.parametrize("nvec", NATIVE_NVEC)
def test_native_golden_fixtures(torch, monkeypatch, name, dtype, tag, nvec):
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    row_ptr, col, val, X, ref = fixture_case(name, tag)
    Y, st = run_multi(torch, spmv_hw.load(dtype), row_ptr, col, val, X, nvec)
    assert st["native"] == 1 and st["kernel"] == 5
    check(row_ptr, col, val, X, ref, Y, dtype)
    if np.dtype(dtype) == np.float64:
        bitwise(Y, ref[:, :nvec])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("nvec", NATIVE_NVEC)
def test_native_fp32_accumulator_is_bitwise_gold(torch, monkeypatch, name, nvec):
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    monkeypatch.setenv("SPMV_SLICE_ACC", "32")
    row_ptr, col, val, X, ref = fixture_case(name, "f32")
    Y, st = run_multi(torch, spmv_hw.load(np.float32), row_ptr, col, val, X, nvec)
    assert st["native"] == 1
    bitwise(Y, ref[:, :nvec])


# ---- 2. shapes where the kernel can go wrong ----
def csr_from_rows(rows, m, dtype, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([len(r) for r in rows], np.int64)
    row_ptr = np.zeros(len(rows) + 1, np.int64)
    row_ptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.uint32)
    assert not len(col) or int(col.max()) < m
    val = rng.uniform(-1, 1, len(col)).astype(dtype)
    return row_ptr.astype(np.uint32), col, val


def band_rows(n, lens, rng, width=40):
    return [np.sort(rng.choice(width, size=int(k), replace=False)) + i for i, k in enumerate(lens[:n])]


def shape_case(case):
    """(rows, nr_cols, format bits that must be set, format bits that must be clear). Format bits
    (spmv_plan_stats.format): 1 narrow offsets, 8 the 8-bit form, 16 the clustered form."""
    rng = np.random.default_rng(sum(map(ord, case)))
    if case.startswith("rows_"):  # 1, 63, 64, 65, 64 * 3 + 5 rows
        n = int(case.split("_")[1])
        return band_rows(n, rng.integers(0, 10, n), rng), n + 40, 0, 0
    if case == "odd_and_long_slices":
        # slice 0: longest row 7 (odd); slice 1: longest row 21 (odd, longer than the 2 * PU
        # entries of an iteration, 8 at the most, at every nvec: full iterations, skipped pairs,
        # the odd slot); slice 2: longest row 18 (even, two full iterations and one pair at PU = 4)
        lens = np.r_[rng.integers(0, 8, 64), rng.integers(0, 22, 64), rng.integers(0, 19, 40)]
        lens[3], lens[70], lens[130] = 7, 21, 18
        return band_rows(len(lens), lens, rng), len(lens) + 40, 0, 0
    if case == "empty_slices":  # a slice of only empty rows, and trailing empty rows
        lens = np.r_[rng.integers(1, 6, 64), np.zeros(64, int), rng.integers(0, 6, 22), np.zeros(50, int)]
        return band_rows(len(lens), lens, rng), len(lens) + 40, 0, 0
    if case == "nnz_0":
        return [np.zeros(0, np.int64)] * 100, 50, 0, 0
    if case == "one_row_of_3000":  # forced slices, heavy padding
        m = 5000
        rows = [np.sort(rng.choice(m, size=int(k), replace=False)) for k in rng.integers(1, 6, 300)]
        rows[70] = np.sort(rng.choice(m, size=3000, replace=False))
        return rows, m, 0, 0
    if case == "offsets_8bit":  # a band under 256 columns
        return [np.sort(rng.choice(150, size=6, replace=False)) + i for i in range(500)], 700, 1 | 8, 16
    if case == "offsets_16bit":  # a span under 65536
        return [np.sort(rng.choice(60_000, size=6, replace=False)) for _ in range(500)], 60_000, 1, 8 | 16
    if case == "offsets_clustered":  # slot 1: two clusters 100 000 columns apart, each under 16384 wide
        return [np.array([i, (i % 2) * 100_000 + i + 7]) for i in range(500)], 110_000, 1 | 16, 8
    if case == "offsets_32bit":  # random columns over 200k
        return [np.sort(rng.choice(200_000, size=6, replace=False)) for _ in range(500)], 200_000, 0, 1 | 8 | 16
    raise KeyError(case)


SHAPES = ["rows_1", "rows_63", "rows_64", "rows_65", "rows_197", "odd_and_long_slices", "empty_slices", "nnz_0",
          "one_row_of_3000", "offsets_8bit", "offsets_16bit", "offsets_clustered", "offsets_32bit"]


@pytest.mark.parametrize("case", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_native_shapes(torch, monkeypatch, case, dtype):
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    rows, m, want, wantnot = shape_case(case)
    row_ptr, col, val = csr_from_rows(rows, m, dtype, seed=1)
    X = make_X(m, dtype, seed=2)
    ref = gold_columns(row_ptr, col, val, X)
    for nvec in NATIVE_NVEC:
        Y, st = run_multi(torch, spmv_hw.load(dtype), row_ptr, col, val, X, nvec)
        assert st["native"] == 1 and st["kernel"] == 5
        assert st["format"] & want == want and not st["format"] & wantnot, (case, st["format"])
        check(row_ptr, col, val, X, ref, Y, dtype)
        if np.dtype(dtype) == np.float64:
            bitwise(Y, ref[:, :nvec])


# ---- 3. padding is masked ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("wide", [False, True])
def test_native_padding_lanes_do_not_leak_nonfinite_x(torch, monkeypatch, dtype, wide):
    """Every slice holds one row of 12 entries among rows of 1-4: in slots 4..11 the long row's
    entry is the slot's only real one, so its column is the slot base that the 63 padding lanes
    gather from. Those rows of X hold NaN and +-Inf, and so does every row of X that no entry
    touches (the 32-bit form's padding reads column 0). The long rows are non-finite by right;
    every other row must be finite and spmv_gold's. wide: columns over 200k (32-bit form)."""
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    rng = np.random.default_rng(11)
    n, m = 64 * 5 + 9, 200_000 if wide else 3000
    short_lo, long_lo = (1, m // 2) if not wide else (1, 100_000)
    rows, poison = [], []
    for i in range(n):
        if i % 64 == 17:  # the slice's long row: columns no short row uses
            c = np.sort(rng.choice(m - long_lo, size=12, replace=False)) + long_lo
            poison += list(c[4:])
        else:
            c = np.sort(rng.choice(long_lo - short_lo, size=int(rng.integers(1, 5)), replace=False)) + short_lo
        rows.append(c)
    row_ptr, col, val = csr_from_rows(rows, m, dtype, seed=3)
    X = make_X(m, dtype, seed=4)
    untouched = np.setdiff1d(np.arange(m), col)
    bad = np.r_[np.array(poison), untouched]
    X[bad] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype), (len(bad), 1))
    assert 0 in untouched
    Xfin = np.where(np.isfinite(X), X, 0).astype(dtype)
    ref = np.stack([oracle.spmv_gold(row_ptr, col, val, np.ascontiguousarray(Xfin[:, j])) for j in range(MAXVEC)], axis=1)
    short = np.arange(n) % 64 != 17
    for nvec in NATIVE_NVEC:
        Y, st = run_multi(torch, spmv_hw.load(dtype), row_ptr, col, val, X, nvec)
        assert st["native"] == 1 and bool(st["format"] & 1) == (not wide)
        assert np.isfinite(Y[short]).all(), "a padding lane's x reached Y"
        assert not np.isfinite(Y[~short]).any()  # 8 non-finite x values per long row
        sub_rp = np.zeros(int(short.sum()) + 1, np.int64)
        lens = np.diff(row_ptr.astype(np.int64))
        sub_rp[1:] = np.cumsum(lens[short])
        keep = np.repeat(short, lens)
        check(sub_rp.astype(np.uint32), col[keep], val[keep], Xfin, ref[short], Y[short], dtype)
        if np.dtype(dtype) == np.float64:
            bitwise(np.ascontiguousarray(Y[short]), np.ascontiguousarray(ref[short][:, :nvec]))


# ---- 5. fallback ----
@functools.lru_cache(maxsize=None)
def powerlaw_case(tag):
    """Power-law n = 20 000, nnz = 320 000 (the size test_abi.py uses), on the host."""
    import torch
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    lib = spmv_hw.load(dtype)
    n, z = 20_000, 320_000
    rp, col, val, _ = spmv_hw.gen_powerlaw(lib, n, n, z, seed=4)
    torch.cuda.synchronize()
    row_ptr, c, v = rp.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32), val.cpu().numpy()
    X = make_X(n, dtype, seed=9)
    return row_ptr, c, v, X, gold_columns(row_ptr, c, v, X)


@pytest.mark.parametrize("kernel", ["tiles", "sweep", "binned", "gold", "blocked"])
@pytest.mark.parametrize("dtype,tag", DTYPES)
@pytest.mark.parametrize("nvec", NATIVE_NVEC)
def test_fallback_forced_kernels(torch, monkeypatch, kernel, dtype, tag, nvec):
    monkeypatch.setenv("SPMV_HW_KERNEL", kernel)
    row_ptr, col, val, X, ref = powerlaw_case(tag)
    Y, st = run_multi(torch, spmv_hw.load(dtype), row_ptr, col, val, X, nvec)
    assert st["native"] == 0 and st["kernel"] == KERNEL_ID[kernel]
    check(row_ptr, col, val, X, ref, Y, dtype)
    if kernel == "gold":
        bitwise(Y, ref[:, :nvec])


@pytest.mark.parametrize("dtype,tag", DTYPES)
@pytest.mark.parametrize("nvec", [1, 3, 5])
def test_fallback_other_vector_counts(torch, monkeypatch, dtype, tag, nvec):
    monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    row_ptr, col, val, X, ref = powerlaw_case(tag)
    Y, st = run_multi(torch, spmv_hw.load(dtype), row_ptr, col, val, X, nvec)
    assert st["native"] == 0
    check(row_ptr, col, val, X, ref, Y, dtype)


@pytest.mark.parametrize("nvec", [1, 3, 7])
def test_forced_slices_with_other_vector_counts_take_the_fallback(torch, monkeypatch, nvec):
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    row_ptr, col, val, X, ref = fixture_case(FIXTURES[0], "f64")
    Y, st = run_multi(torch, spmv_hw.load(np.float64), row_ptr, col, val, X, nvec)
    assert st["native"] == 0 and st["kernel"] == 5
    bitwise(Y, ref[:, :nvec])  # kernel 5 per vector: still spmv_gold's bits


# ---- 6. automatic choice ----
def _stencil(points, dtype):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from ab_variants import stencil
    return stencil(46 ** 3, points, dtype)


@pytest.mark.parametrize("matrix", ["banded", "stencil7", "stencil27", "powerlaw"])
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_automatic_choice(torch, monkeypatch, matrix, dtype, tag):
    """Banded and stencil matrices of ~100k rows take the native path at nvec 2, 4 and 8; the
    power-law matrix (slice padding far above the limit) takes the fallback. Y is the oracle's."""
    monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    lib = spmv_hw.load(dtype)
    if matrix == "powerlaw":
        row_ptr, c, v, X, ref = powerlaw_case(tag)
    else:
        if matrix == "banded":
            n = 100_000
            rp, col, val = spmv_hw.gen_banded(lib, n, 16, seed=2)
        else:
            rp, col, val, n = _stencil(int(matrix[7:]), dtype)
        row_ptr, c, v = rp.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32), val.cpu().numpy()
        X = make_X(n, dtype, seed=5)
        ref = gold_columns(row_ptr, c, v, X)
    for nvec in NATIVE_NVEC:
        Y, st = run_multi(torch, lib, row_ptr, c, v, X, nvec)
        assert st["native"] == (0 if matrix == "powerlaw" else 1), (matrix, nvec, st)
        check(row_ptr, c, v, X, ref, Y, dtype)
        if st["native"] and np.dtype(dtype) == np.float64:
            bitwise(Y, ref[:, :nvec])


# ---- 7. 64-bit indexing ----
def test_native_indexes_X_past_2_to_the_32(torch, monkeypatch):
    """fp32, nvec = 8, 2^29 + 64 columns: col * 8 passes 2^32 for the last 64 columns. 128 rows
    with entries in the first 64 and the last 64 columns; only those rows of X are set (the rest
    of the 17 GB is zero). The oracle runs on the same matrix with the columns remapped to 128."""
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    monkeypatch.delenv("SPMV_SLICE_ACC", raising=False)
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        print(f"skipped: {free / 2 ** 30:.1f} GB free, the test needs 24 GB")
        pytest.skip(f"{free / 2 ** 30:.1f} GB of device memory free, the test needs 24 GB")
    dtype, nvec, m = np.float32, 8, 2 ** 29 + 64
    rng = np.random.default_rng(13)
    rows_small = [np.r_[np.sort(rng.choice(64, size=3, replace=False)), 64 + np.sort(rng.choice(64, size=3, replace=False))]
                  for _ in range(128)]
    rows_big = [np.where(r < 64, r, r - 64 + (m - 64)) for r in rows_small]
    row_ptr, col_small, val = csr_from_rows(rows_small, 128, dtype, seed=14)
    _, col_big, _ = csr_from_rows(rows_big, m, dtype, seed=14)
    Xs = make_X(128, dtype, seed=15)
    ref = gold_columns(row_ptr, col_small, val, Xs)
    lib = spmv_hw.load(dtype)
    mp = build(torch, lib, row_ptr, col_big, val, m, nvec)
    X = torch.zeros((m, nvec), dtype=torch.float32, device="cuda")
    X[:64] = to_dev(torch, Xs[:64])
    X[m - 64:] = to_dev(torch, Xs[64:])
    Y = torch.full((128, nvec), float("nan"), dtype=torch.float32, device="cuda")
    mp.run(X, Y)
    torch.cuda.synchronize()
    st = mp.stats()
    mp.destroy()
    del X
    torch.cuda.empty_cache()
    assert st["native"] == 1 and st["nr_cols"] == m
    check(row_ptr, col_small, val, Xs, ref, Y.cpu().numpy(), dtype)


# ---- 8. graph capture ----
@pytest.mark.parametrize("path", ["native", "fallback"])
def test_run_is_capturable(torch, monkeypatch, path):
    """MultiPlan.run captured with torch.cuda.graph on one stream and replayed twice."""
    if path == "native":
        monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    else:
        monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    dtype, nvec = np.float64, 4
    row_ptr, col, val, X, ref = powerlaw_case("f64")
    n = len(row_ptr) - 1
    mp = build(torch, spmv_hw.load(dtype), row_ptr, col, val, n, nvec)
    assert mp.stats()["native"] == (1 if path == "native" else 0)
    Xd = to_dev(torch, X[:, :nvec])
    Y = torch.full((n, nvec), float("nan"), dtype=Xd.dtype, device="cuda")
    mp.run(Xd, Y)
    torch.cuda.synchronize()
    eager = Y.cpu().numpy()
    check(row_ptr, col, val, X, ref, eager, dtype)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mp.run(Xd, Y)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mp.run(Xd, Y)
    for _ in range(2):
        Y.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        out = Y.cpu().numpy()
        check(row_ptr, col, val, X, ref, out, dtype)
        if path == "native":
            bitwise(out, eager)
    del g
    mp.destroy()


# ---- argument checks that need a handle ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_run_refuses_misaligned_and_misshapen_tensors(torch, monkeypatch, dtype):
    monkeypatch.setenv("SPMV_HW_KERNEL", "slices")
    row_ptr, col, val, X, _ = fixture_case(FIXTURES[0], "f64" if dtype == np.float64 else "f32")
    n, m, nvec = len(row_ptr) - 1, X.shape[0], 4
    mp = build(torch, spmv_hw.load(dtype), row_ptr, col, val, m, nvec)
    td = spmv_hw._torch_dtype(dtype)
    Xd = to_dev(torch, X[:, :nvec])
    Y = torch.full((n, nvec), float("nan"), dtype=td, device="cuda")
    # one value into a buffer: aligned to sizeof(ValueType) only, the call needs min(16, 4 * sizeof)
    Xoff = torch.zeros(m * nvec + 1, dtype=td, device="cuda")[1:].view(m, nvec)
    Yoff = torch.zeros(n * nvec + 1, dtype=td, device="cuda")[1:].view(n, nvec)
    for a, b in ((Xoff, Y), (Xd, Yoff)):
        with pytest.raises(RuntimeError, match="misaligned"):
            mp.run(a, b)
    with pytest.raises(ValueError, match="shape"):
        mp.run(Xd[:, :2].contiguous(), Y)
    with pytest.raises(ValueError, match="shape"):
        mp.run(Xd, Y[:-1])
    with pytest.raises(ValueError, match="contiguous"):
        mp.run(to_dev(torch, np.ascontiguousarray(X[:, :nvec].T)).t(), Y)
    with pytest.raises(ValueError, match="library is"):
        mp.run(Xd.to(torch.float16), Y)
    torch.cuda.synchronize()
    assert torch.isnan(Y).all()  # nothing was enqueued
    mp.run(Xd, Y)
    torch.cuda.synchronize()
    assert not torch.isnan(Y).any()
    mp.destroy()
