"""The eight create paths -- {Plan, MultiPlan} x {from_host, from_device} x {N, T} -- on the same
row slice of one matrix (GPU). Every path goes through one slice descriptor:
filled from a host matrix and a row range, or from device arrays whose row_ptr starts at an
offset. Each must multiply by that slice (or its transpose), report its shape, and the host- and
the device-created plan of one slice must agree bit for bit where the order of additions is fixed.

The matrix has the shape tests/test_sanitize.py generates: 300 x 200, about 2000 entries, the last
20 rows empty, columns unsorted within rows. The slices are [37, 229) (neither bound a multiple
of the 64-row slice height, first entry not at 0) and the empty [5, 5)."""
import functools

import numpy as np
import pytest

import oracle
import spmv_hw
from conftest import DTYPES
from test_gpu_multi import check as check_columns
from test_gpu_transpose import check as check_vector, np_transpose, to_dev, torch  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N, M, Z = 300, 200, 2000
NVEC = 2
RANGE, EMPTY = (37, 229), (5, 5)
PATHS = [(obj, src, tr) for obj in ("plan", "multi") for src in ("host", "device") for tr in (False, True)]
PATH_IDS = [f"{obj}-{src}-{'T' if tr else 'N'}" for obj, src, tr in PATHS]


@functools.lru_cache(maxsize=None)
def matrix(tag):
    dtype = dict((t, d) for d, t in DTYPES)[tag]
    rng = np.random.default_rng(3)
    rows = np.sort(rng.integers(0, N - 20, Z))
    col = rng.integers(0, M, Z).astype(np.uint32)
    val = rng.uniform(-10, 10, Z).astype(dtype)
    row_ptr = np.zeros(N + 1, np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    assert np.all(np.diff(row_ptr)[280:] == 0) and np.any(np.diff(col.astype(np.int64))[:50] < 0)
    return row_ptr.astype(np.uint32), col, val


@functools.lru_cache(maxsize=None)
def reference(tag, r0, r1, transpose):
    """(row_ptr, col, val) of the slice or of its numpy transpose, X for it (NVEC columns) and the
    oracle's product with every column."""
    row_ptr, col, val = matrix(tag)
    b, e = int(row_ptr[r0]), int(row_ptr[r1])
    rp, c, v = (row_ptr[r0:r1 + 1] - row_ptr[r0]).astype(np.uint32), col[b:e], val[b:e]
    if transpose:
        rp, c, v = np_transpose(rp, c, v, M)
    X = np.random.default_rng(r0 + 2 * transpose).uniform(0, 1, (r1 - r0 if transpose else M, NVEC)).astype(val.dtype)
    ref = np.stack([oracle.spmv_gold(rp, c, v, np.ascontiguousarray(X[:, j])) for j in range(NVEC)], axis=1)
    return rp, c, v, X, ref


def create(torch, lib, tag, obj, src, transpose, r0, r1):
    row_ptr, col, val = matrix(tag)
    cls, nvec = (spmv_hw.Plan, ()) if obj == "plan" else (spmv_hw.MultiPlan, (NVEC,))
    if src == "host":
        return cls.from_host(lib, lib.make_csr_matrix(row_ptr, col, val, M), r0, r1, *nvec, transpose=transpose)
    # row_ptr[r0 .. r1] as it stands in the whole matrix's array, with the whole col / val
    d_rp, d_col, d_val = (to_dev(torch, a) for a in (row_ptr, col, val))
    return cls.from_device(lib, d_rp[r0:r1 + 1], d_col, d_val, M, *nvec, transpose=transpose)


def run(torch, p, X, rows):
    """Y (rows, columns of X) of one run, pre-filled NaN. A vector without elements is passed as a
    one-element buffer: the C functions refuse a null x when there are rows to write."""
    k = X.shape[1]
    dt = spmv_hw._torch_dtype(p.lib.dtype)
    Xd = to_dev(torch, X if len(X) else np.zeros((1, k), X.dtype))
    Y = torch.full((max(rows, 1), k), float("nan"), dtype=dt, device="cuda")
    if isinstance(p, spmv_hw.Plan):
        p.run(Xd, Y)
    else:
        p.lib._ok(p.lib.L.spmv_multi_run(p.h, Xd.data_ptr(), Y.data_ptr(), None), "spmv_multi_run")
    torch.cuda.synchronize()
    return Y.cpu().numpy()[:rows]


def shape(r0, r1, transpose):
    row_ptr = matrix("f64")[0]
    n, z = r1 - r0, int(row_ptr[r1]) - int(row_ptr[r0])
    return (M, n, z) if transpose else (n, M, z)


@pytest.mark.parametrize("obj,src,transpose", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_every_create_path_multiplies_by_the_slice(torch, monkeypatch, dtype, tag, obj, src, transpose):
    monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    lib = spmv_hw.load(dtype)
    r0, r1 = RANGE
    rp, c, v, X, ref = reference(tag, r0, r1, transpose)
    p = create(torch, lib, tag, obj, src, transpose, r0, r1)
    st = p.stats()
    assert (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == shape(r0, r1, transpose), st
    assert p.op == (spmv_hw.OP_T if transpose else spmv_hw.OP_N)
    k = 1 if obj == "plan" else NVEC
    assert obj == "plan" or st["nvec"] == NVEC
    Y = run(torch, p, X[:, :k], len(rp) - 1)
    p.destroy()
    if obj == "plan":
        check_vector(rp, c, v, *(np.ascontiguousarray(a[:, 0]) for a in (X, ref, Y)), dtype, False)
    else:
        check_columns(rp, c, v, X, ref, Y, dtype)


@pytest.mark.parametrize("transpose", [False, True], ids=["N", "T"])
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_host_and_device_created_plans_agree_bit_for_bit(torch, monkeypatch, dtype, tag, transpose):
    """SPMV_HW_KERNEL=gold fixes the order of additions: both plans give spmv_gold's bits."""
    monkeypatch.setenv("SPMV_HW_KERNEL", "gold")
    lib = spmv_hw.load(dtype)
    r0, r1 = RANGE
    rp, c, v, X, ref = reference(tag, r0, r1, transpose)
    got = {}
    for src in ("host", "device"):
        p = create(torch, lib, tag, "plan", src, transpose, r0, r1)
        assert p.stats()["kernel"] == 1
        got[src] = np.ascontiguousarray(run(torch, p, X[:, :1], len(rp) - 1)[:, 0])
        p.destroy()
    assert got["host"].tobytes() == got["device"].tobytes()
    check_vector(rp, c, v, np.ascontiguousarray(X[:, 0]), np.ascontiguousarray(ref[:, 0]), got["host"], dtype, True)


@pytest.mark.parametrize("obj,src,transpose", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("dtype,tag", DTYPES)
def test_empty_row_range(torch, monkeypatch, dtype, tag, obj, src, transpose):
    """[5, 5): no rows (N) or no columns (T). Creates, runs and destroys; A^T x of no rows is 0."""
    monkeypatch.delenv("SPMV_HW_KERNEL", raising=False)
    lib = spmv_hw.load(dtype)
    r0, r1 = EMPTY
    p = create(torch, lib, tag, obj, src, transpose, r0, r1)
    st = p.stats()
    assert (st["nr_rows"], st["nr_cols"], st["nr_nzeros"]) == shape(r0, r1, transpose) == ((M, 0, 0) if transpose else (0, M, 0))
    k = 1 if obj == "plan" else NVEC
    X = np.ones((0 if transpose else M, k), dtype)
    Y = run(torch, p, X, st["nr_rows"])
    p.destroy()
    assert Y.shape == (st["nr_rows"], k) and not Y.any() and not np.isnan(Y).any()
