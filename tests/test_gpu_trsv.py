"""Sparse triangular solve on the GPU (spmv_trsv_*, spmv_hw.TriSolve), both precisions,
LOWER and -- through the reversed permutation of the same matrix (row i -> n - 1 - i, column c ->
n - 1 - c) -- UPPER.

Correctness rule (derived, not measured). Substitution in any summation order is componentwise
backward stable (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5): for every row i
with k_i stored entries in the triangle, |b - T x|_i <= 2 (k_i + 3) u (|T| |x| + |b|)_i with
u = 2^-53 (fp64) or 2^-24 (fp32), the left side evaluated in float64 (the factor 2 covers that
evaluation's own rounding when the data are fp64), and every x_i finite. The generators make every
row diagonally dominant, |t_ii| >= 1 + sum |t_ij|, so x stays bounded."""
import functools

import numpy as np
import pytest

import spmv_hw

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
UPLO = ["lower", "upper"]
CUT = 32        # kTrsvLongRow: rows with more off-diagonal entries take the wave form
CHAIN = 1024    # kTrsvChainRows


# ---------------------------------------------------------------- helpers

def dev(h):
    import torch
    return torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).cuda()


def csr_from_rows(rows, cols, vals, n):
    """CSR of entries already grouped by row in the wanted order (rows non-decreasing)."""
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rp.astype(np.uint32), cols.astype(np.uint32), vals


def row_ids(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp.astype(np.int64)))


def reversed_matrix(rp, col, val):
    """P A P^T for the reversal P: a lower triangle becomes an upper one; the entries of a row keep
    their CSR order."""
    n = len(rp) - 1
    rows = n - 1 - row_ids(rp)
    order = np.argsort(rows, kind="stable")
    return csr_from_rows(rows[order], (n - 1 - col.astype(np.int64))[order], val[order], n)


def oriented(mat, uplo):
    """The (lower-triangular or full) matrix for LOWER, its reversal for UPPER."""
    return mat if uplo == "lower" else reversed_matrix(*mat)


def reverse_vec(v, uplo):
    return v if uplo == "lower" else v[::-1].copy()


def check_rule(rp, col, val, lower, unit, b, x, dtype, what=""):
    """The correctness rule of the module docstring; every stored entry of the triangle counts on its
    own (duplicates are not merged). Prints the worst ratio residual / bound before asserting."""
    n = len(rp) - 1
    rows, c = row_ids(rp), col.astype(np.int64)
    keep = ((c < rows) if lower else (c > rows)) | ((c == rows) & (not unit))
    rows, c, v = rows[keep], c[keep], val[keep].astype(np.float64)
    x64, b64 = x.astype(np.float64), b.astype(np.float64)
    assert np.isfinite(x64).all(), f"{what}: x is not finite"
    prod = v * x64[c]
    tx = np.bincount(rows, prod, n)
    mag = np.bincount(rows, np.abs(prod), n)
    k = np.bincount(rows, minlength=n).astype(np.float64)
    if unit:
        tx, mag, k = tx + x64, mag + np.abs(x64), k + 1
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    bound = 2.0 * (k + 3.0) * u * (mag + np.abs(b64))
    res = np.abs(b64 - tx)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, res / bound, np.where(res > 0, np.inf, 0.0))
    print(f"{what} {np.dtype(dtype).name}: worst residual / bound = {ratio.max() if n else 0.0:.3f}")
    assert (res <= bound).all(), f"{what}: worst residual / bound {ratio.max():.3f} at row {int(ratio.argmax())}"


def solve(lib, mat, b, lower, unit=False, in_place=False, keep=False):
    """x (numpy) and the stats of a handle built from the device copy of mat."""
    import torch
    rp, col, val = mat
    n = len(rp) - 1
    t = spmv_hw.TriSolve.from_device(lib, dev(rp), dev(col), dev(val.astype(lib.dtype)), n, lower=lower,
                                     unit_diag=unit)
    d_b = dev(b.astype(lib.dtype))
    d_x = d_b if in_place else torch.full_like(d_b, float("nan"))
    t.solve(d_b, d_x)
    torch.cuda.synchronize()
    x, st = d_x.cpu().numpy(), t.stats()
    if keep:
        return x, st, t
    t.destroy()
    return x, st


def dominant_diag(rp, col, val, dtype, rng):
    """Adds a diagonal entry of magnitude 1 + sum |row| (random sign) at the end of each row of a
    strictly triangular matrix whose values are already rounded to dtype."""
    n = len(rp) - 1
    rows = row_ids(rp)
    mag = 1.0 + np.bincount(rows, np.abs(val), n)
    d = (mag * rng.choice([-1.0, 1.0], n)).astype(dtype).astype(np.float64)
    all_rows = np.concatenate([rows, np.arange(n)])
    order = np.argsort(all_rows, kind="stable")  # the diagonal lands last in its row
    return csr_from_rows(all_rows[order], np.concatenate([col.astype(np.int64), np.arange(n)])[order],
                         np.concatenate([val, d])[order], n)


@functools.lru_cache(maxsize=None)
def random_lower(n, per, dtype_name, seed=3):
    """Row i: min(i, per) entries at random columns < i (repeats possible), then the dominant diagonal."""
    rng = np.random.default_rng(seed)
    cnt = np.minimum(np.arange(n), per)
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    cols = (rng.random(len(rows)) * rows).astype(np.int64)
    vals = rng.uniform(-1, 1, len(rows)).astype(dtype_name).astype(np.float64)
    rp, col, val = csr_from_rows(rows, cols, vals, n)
    return dominant_diag(rp, col, val, dtype_name, rng)


@functools.lru_cache(maxsize=None)
def grid_matrix(g, red_black, lower_only):
    """5-point grid, diagonal 4.125 and -1 off it (dominant in each triangle), columns sorted; values
    exact in fp32. red_black: the points with i + j even first."""
    n = g * g
    idx = np.arange(n, dtype=np.int64)
    i, j = idx // g, idx % g
    new = idx
    if red_black:
        black = (i + j) % 2 == 1
        new = np.empty(n, np.int64)
        new[~black] = np.arange(int((~black).sum()))
        new[black] = int((~black).sum()) + np.arange(int(black.sum()))
    rows, cols, vals = [], [], []
    for o, ok in ((-g, i > 0), (-1, j > 0), (0, np.ones(n, bool)), (1, j < g - 1), (g, i < g - 1)):
        rows.append(new[idx[ok]])
        cols.append(new[idx[ok] + o])
        vals.append(np.full(int(ok.sum()), 4.125 if o == 0 else -1.0))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    if lower_only:
        keep = cols <= rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    return csr_from_rows(rows[order], cols[order], vals[order], n)


def rhs(n, seed=11):
    return np.random.default_rng(seed).uniform(-1, 1, n)


# ---------------------------------------------------------------- 1. exact results

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_diagonal_matrix_is_bitwise_b_over_d(dtype, uplo):
    lib = spmv_hw.load(dtype)
    n = 1000
    rng = np.random.default_rng(1)
    d = (rng.uniform(1, 2, n) * rng.choice([-1, 1], n)).astype(dtype)
    b = rhs(n).astype(dtype)
    mat = (np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), d)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert np.array_equal(x, b / d)
    assert (st["nr_levels"], st["nr_launches"], st["nr_chain_levels"], st["nr_nzeros"]) == (1, 1, 1, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_unit_diagonal_without_off_diagonals_is_bitwise_b(dtype, uplo):
    lib = spmv_hw.load(dtype)
    n = 1000
    b = rhs(n).astype(dtype)
    stored = (np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), np.full(n, 7.0))  # ignored
    empty = (np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0))
    for mat in (stored, empty):
        x, st = solve(lib, mat, b, uplo == "lower", unit=True)
        assert np.array_equal(x, b)
        assert st["nr_nzeros"] == 0 and st["diag"] == spmv_hw.TRSV_DIAG_UNIT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_bidiagonal_chain_counts_exactly(dtype, uplo):
    """diag 1, subdiagonal -1, b = 1: x_i = i + 1 exactly. 3000 levels of one row in ONE chain launch:
    every level reads the x its predecessor wrote, across the chain kernel's barrier, from a cache
    line it has read before -- a stale read shows as a wrong integer."""
    lib = spmv_hw.load(dtype)
    n = 3000
    rows = np.concatenate([[0], np.repeat(np.arange(1, n), 2)])
    cols = np.concatenate([[0], np.stack([np.arange(n - 1), np.arange(1, n)], 1).ravel()])
    vals = np.concatenate([[1.0], np.tile([-1.0, 1.0], n - 1)])
    mat = oriented(csr_from_rows(rows, cols, vals, n), uplo)
    x, st = solve(lib, mat, np.ones(n), uplo == "lower")
    assert np.array_equal(reverse_vec(x, uplo), np.arange(1, n + 1).astype(dtype))
    assert (st["nr_levels"], st["nr_launches"], st["nr_chain_levels"], st["max_level_rows"]) == (n, 1, n, 1)


# ---------------------------------------------------------------- 2. grid: chain, wide launches, chain

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_grid_natural_order_mixes_chain_and_wide_launches(dtype, uplo):
    lib = spmv_hw.load(dtype)
    g = 1500
    mat = oriented(grid_matrix(g, False, True), uplo)
    b = rhs(g * g).astype(dtype)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert st["nr_levels"] == 2 * g - 1 and st["max_level_rows"] == g
    assert st["nr_launches"] < st["nr_levels"] and st["nr_chain_levels"] > 0
    # widths 1..g..1: the 2 * CHAIN narrow levels are two chain launches, every other level a launch
    assert st["nr_chain_levels"] == 2 * CHAIN and st["nr_launches"] == 2 + (2 * g - 1 - 2 * CHAIN)
    check_rule(*mat, uplo == "lower", False, b, x, dtype, f"grid natural {uplo}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_grid_red_black_order_has_two_levels(dtype, uplo):
    lib = spmv_hw.load(dtype)
    g = 1500
    mat = oriented(grid_matrix(g, True, True), uplo)
    b = rhs(g * g).astype(dtype)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert st["nr_levels"] == 2 and st["nr_launches"] == 2 and st["nr_chain_levels"] == 0
    check_rule(*mat, uplo == "lower", False, b, x, dtype, f"grid red-black {uplo}")


# ---------------------------------------------------------------- 3. random triangle

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_random_triangle(dtype, uplo):
    lib = spmv_hw.load(dtype)
    n = 200_000
    mat = oriented(random_lower(n, 12, np.dtype(dtype).name), uplo)
    b = rhs(n).astype(dtype)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert st["nr_levels"] > 2 and st["max_level_rows"] > CHAIN and st["nr_chain_levels"] > 0
    assert st["nr_nzeros"] == int(mat[0][-1])
    check_rule(*mat, uplo == "lower", False, b, x, dtype, f"random {uplo}")


# ---------------------------------------------------------------- 4. long rows (wave per row)

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_arrow_matrix_dense_last_row(dtype, uplo):
    lib = spmv_hw.load(dtype)
    n = 5000
    rng = np.random.default_rng(5)
    rows = np.full(n - 1, n - 1, np.int64)
    vals = rng.uniform(-1, 1, n - 1).astype(dtype).astype(np.float64)
    low = dominant_diag(*csr_from_rows(rows, np.arange(n - 1), vals, n), dtype, rng)
    mat = oriented(low, uplo)
    b = rhs(n).astype(dtype)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert (st["nr_levels"], st["nr_launches"], st["nr_chain_levels"]) == (2, 2, 1)  # 4999 rows wide, 1 row chain
    check_rule(*mat, uplo == "lower", False, b, x, dtype, f"arrow {uplo}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_row_lengths_around_the_long_cut_in_a_wide_and_a_narrow_level(dtype, uplo):
    """Level 0: 2000 diagonal rows. Level 1 (1200 rows, a wide launch) and level 2 (70 rows, a chain
    launch): off-diagonal counts cycling through CUT - 1, CUT, CUT + 1, 63, 64, 65, 129, at distinct
    random columns of the level before."""
    lib = spmv_hw.load(dtype)
    rng = np.random.default_rng(9)
    lengths = [CUT - 1, CUT, CUT + 1, 63, 64, 65, 129]
    n0, n1, n2 = 2000, 1200, 70
    n = n0 + n1 + n2
    rows, cols = [], []
    for first, count, (lo, hi) in ((n0, n1, (0, n0)), (n0 + n1, n2, (n0, n0 + n1))):
        for k in range(count):
            ln = lengths[k % len(lengths)]
            rows.append(np.full(ln, first + k, np.int64))
            cols.append(rng.choice(np.arange(lo, hi), ln, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(-1, 1, len(rows)).astype(dtype).astype(np.float64)
    low = dominant_diag(*csr_from_rows(rows, cols, vals, n), dtype, rng)
    mat = oriented(low, uplo)
    b = rhs(n).astype(dtype)
    x, st = solve(lib, mat, b, uplo == "lower")
    assert (st["nr_levels"], st["nr_launches"], st["nr_chain_levels"], st["max_level_rows"]) == (3, 3, 1, n0)
    check_rule(*mat, uplo == "lower", False, b, x, dtype, f"long rows {uplo}")


# ---------------------------------------------------------------- 5. a full matrix passed whole

@pytest.mark.parametrize("dtype", DTYPES)
def test_full_symmetric_matrix_equals_its_extracted_triangles_bitwise(dtype):
    lib = spmv_hw.load(dtype)
    g = 300
    full = grid_matrix(g, False, False)
    rp, col, val = full
    rows, c = row_ids(rp), col.astype(np.int64)
    b = rhs(g * g).astype(dtype)
    for lower in (True, False):
        keep = (c <= rows) if lower else (c >= rows)
        tri = csr_from_rows(rows[keep], c[keep], val[keep], g * g)
        x_full, st_full = solve(lib, full, b, lower)
        x_tri, st_tri = solve(lib, tri, b, lower)
        assert np.array_equal(x_full, x_tri)
        assert st_full == st_tri and st_full["nr_nzeros"] == int(tri[0][-1])
        check_rule(*full, lower, False, b, x_full, dtype, f"full grid lower={lower}")
    # row_ptr starting at an offset into longer arrays: the same bits
    pad = 5
    rp_off = (rp.astype(np.int64) + pad).astype(np.uint32)
    col_off = np.concatenate([np.full(pad, 2 ** 31 - 1, np.uint32), col])
    val_off = np.concatenate([np.full(pad, np.nan), val])
    x_off, _ = solve(lib, (rp_off, col_off, val_off), b, True)
    assert np.array_equal(x_off, solve(lib, full, b, True)[0])


# ---------------------------------------------------------------- 6. unsorted columns, duplicates

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_unsorted_columns_and_duplicate_entries(dtype, uplo):
    """Every row's entries shuffled, every third off-diagonal entry and every diagonal stored twice
    (the same value again, so the canonical matrix -- columns sorted, duplicates summed -- is exact:
    2 a, and |T| is the same operator). The rule is evaluated on the duplicated entries, which is the
    rule of the canonical matrix with the larger k_i of the stored entries; the canonical handle
    meets its own. A UNIT handle ignores the stored diagonal."""
    lib = spmv_hw.load(dtype)
    n = 20_000
    rng = np.random.default_rng(13)
    cnt = np.minimum(np.arange(n), 8)
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    cols = (rng.random(len(rows)) * rows).astype(np.int64)
    first = np.unique(rows * n + cols)  # no chance repeats: the only duplicates are the exact ones below
    rows, cols = first // n, first % n
    vals = rng.uniform(-1, 1, len(rows)).astype(dtype).astype(np.float64)
    twice = np.arange(len(rows)) % 3 == 0
    o_rows = np.concatenate([rows, rows[twice]])
    o_cols = np.concatenate([cols, cols[twice]])
    o_vals = np.concatenate([vals, vals[twice]])
    half = ((1.0 + np.bincount(o_rows, np.abs(o_vals), n)) / 2).astype(dtype).astype(np.float64)
    d_rows = np.repeat(np.arange(n, dtype=np.int64), 2)
    a_rows = np.concatenate([o_rows, d_rows])
    a_cols = np.concatenate([o_cols, d_rows])
    a_vals = np.concatenate([o_vals, np.repeat(half, 2)])
    shuffle = np.lexsort((rng.random(len(a_rows)), a_rows))  # rows grouped, entries in random order
    dup = oriented(csr_from_rows(a_rows[shuffle], a_cols[shuffle], a_vals[shuffle], n), uplo)
    # canonical: sorted by (row, column), equal (row, column) summed
    key = a_rows * n + a_cols
    uniq, inv = np.unique(key, return_inverse=True)
    canon = oriented(csr_from_rows(uniq // n, uniq % n, np.bincount(inv, a_vals), n), uplo)
    assert len(canon[1]) < len(dup[1])
    b = rhs(n).astype(dtype)
    lower = uplo == "lower"
    x_dup, st_dup = solve(lib, dup, b, lower)
    x_can, st_can = solve(lib, canon, b, lower)
    assert st_dup["nr_levels"] == st_can["nr_levels"] and st_dup["nr_nzeros"] == len(dup[1])
    check_rule(*dup, lower, False, b, x_dup, dtype, f"duplicates {uplo}")
    check_rule(*canon, lower, False, b, x_can, dtype, f"canonical {uplo}")
    # UNIT: the stored diagonal is ignored -- the same bits as without it
    rows_d, c_d = row_ids(dup[0]), dup[1].astype(np.int64)
    off = c_d != rows_d
    no_diag = csr_from_rows(rows_d[off], c_d[off], dup[2][off] / 16, n)  # /16: x stays bounded under a unit diagonal
    with_diag = (dup[0], dup[1], np.where(off, dup[2] / 16, dup[2]))
    x_u, st_u = solve(lib, with_diag, b, lower, unit=True)
    x_n, _ = solve(lib, no_diag, b, lower, unit=True)
    assert np.array_equal(x_u, x_n) and st_u["nr_nzeros"] == len(no_diag[1])
    check_rule(*with_diag, lower, True, b, x_u, dtype, f"unit {uplo}")


# ---------------------------------------------------------------- 7. reproducibility and aliasing

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("uplo", UPLO)
def test_runs_and_handles_are_bitwise_reproducible_and_in_place_is_allowed(dtype, uplo):
    import torch
    lib = spmv_hw.load(dtype)
    n = 200_000
    mat = oriented(random_lower(n, 12, np.dtype(dtype).name), uplo)
    b = rhs(n).astype(dtype)
    lower = uplo == "lower"
    x1, _, t = solve(lib, mat, b, lower, keep=True)
    d_b = dev(b)
    d_x = torch.full_like(d_b, float("nan"))
    t.solve(d_b, d_x)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy(), x1)  # a second run of the handle
    t.destroy()
    assert np.array_equal(solve(lib, mat, b, lower)[0], x1)  # a second handle of the same input
    assert np.array_equal(solve(lib, mat, b, lower, in_place=True)[0], x1)  # solve(b, b)


# ---------------------------------------------------------------- 8. graph capture

@pytest.mark.parametrize("dtype", DTYPES)
def test_lower_then_upper_solve_captured_in_a_graph(dtype):
    """A LOWER and an UPPER solve of one symmetric matrix (T + T^T of a random triangle: wide levels
    and a narrow tail in each handle) captured on a side stream after one warm-up run; each of 3
    replays gives the eager run's bits."""
    import scipy.sparse as sp
    import torch
    lib = spmv_hw.load(dtype)
    n = 50_000
    rp, col, val = random_lower(n, 4, np.dtype(dtype).name, seed=21)
    T = sp.csr_matrix((val, col.astype(np.int64), rp.astype(np.int64)), shape=(n, n))
    T.sum_duplicates()
    S = sp.tril(T, -1) + sp.tril(T, -1).T
    S = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    S.sort_indices()
    S.data = S.data.astype(dtype)
    d = (dev(S.indptr.astype(np.uint32)), dev(S.indices.astype(np.uint32)), dev(S.data))
    lo = spmv_hw.TriSolve.from_device(lib, *d, n, lower=True)
    up = spmv_hw.TriSolve.from_device(lib, *d, n, lower=False)
    assert lo.stats()["nr_launches"] > 2 and lo.stats()["nr_chain_levels"] > 0
    d_b = dev(rhs(n).astype(dtype))
    d_t = torch.full_like(d_b, float("nan"))
    d_x = torch.full_like(d_b, float("nan"))

    def both():
        lo.solve(d_b, d_t)
        up.solve(d_t, d_x)

    both()
    torch.cuda.synchronize()
    eager = d_x.cpu().numpy().copy()
    check_rule(S.indptr.astype(np.uint32), S.indices.astype(np.uint32), S.data, False, False, d_t.cpu().numpy(), eager,
               dtype, "graph upper")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(3):
        d_t.fill_(float("nan"))
        d_x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_x.cpu().numpy(), eager)
    lo.destroy()
    up.destroy()


# ---------------------------------------------------------------- 9. refusals at create, empty handle

@pytest.mark.parametrize("dtype", DTYPES)
def test_create_refusals_and_the_empty_handle(dtype):
    import torch
    lib = spmv_hw.load(dtype)
    n = 50
    rows = np.concatenate([np.arange(1, n), np.delete(np.arange(n), [7, 11])])
    cols = np.concatenate([np.arange(n - 1), np.delete(np.arange(n), [7, 11])])
    order = np.lexsort((cols, rows))
    mat = csr_from_rows(rows[order], cols[order], np.where(rows == cols, 2.0, 0.5)[order], n)
    b = rhs(n).astype(dtype)
    with pytest.raises(RuntimeError, match=r"missing diagonal in row 7\b"):
        solve(lib, mat, b, True)
    with pytest.raises(RuntimeError, match=r"missing diagonal in row 38\b"):  # n - 1 - 11: the first one reversed
        solve(lib, reversed_matrix(*mat), b, False)
    x, _ = solve(lib, mat, b, True, unit=True)  # the same matrix is fine under a unit diagonal
    check_rule(*mat, True, True, b, x, dtype, "unit, no stored diagonal")
    m = lib.make_csr_matrix(*mat, n)  # the host form refuses it the same way
    with pytest.raises(RuntimeError, match=r"missing diagonal in row 7\b"):
        spmv_hw.TriSolve.from_host(lib, m)
    t = spmv_hw.TriSolve.from_host(lib, m, unit_diag=True)
    d_b = dev(b)
    d_x = torch.empty_like(d_b)
    t.solve(d_b, d_x)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy(), x)
    assert lib.L.spmv_trsv_solve(t.h, None, d_x.data_ptr(), None) != 0  # a null b with n > 0
    assert "null argument" in lib.L.spmv_hw_last_error().decode()
    t.destroy()
    bad = (mat[0], mat[1].copy(), mat[2])
    bad[1][3] = n  # a column index >= n, in the other triangle or not
    with pytest.raises(RuntimeError, match="column index out of range"):
        solve(lib, bad, b, True, unit=True)
    # n = 0: an empty handle, its solve a no-op
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    e = spmv_hw.TriSolve.from_device(lib, z, z, torch.zeros(1, dtype=d_b.dtype, device="cuda"), 0)
    assert e.stats()["nr_launches"] == 0
    e.solve(d_b[:0], d_x[:0])
    e.destroy()
