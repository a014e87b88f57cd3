// Host-only check of the triangular solve's planner (spmv-fpga_amd/csrc/trsv_plan.cpp, DESIGN.md
// §16): plan_trsv and build_trsv_layout on small matrices, each as a LOWER problem and, through the
// reversed permutation (row i -> n - 1 - i, column c -> n - 1 - c), as an UPPER one. Built with
// -fsanitize=address,undefined by the Makefile beside it; tests/test_trsv_host.py runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "spmv_host.hpp"

using namespace spmvhw;

struct entry {
    IndexType c;
    ValueType v;
};
typedef std::vector<std::vector<entry>> matrix;  // rows of (column, value), in CSR order

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            std::fprintf(stderr, "FAILED %s (%s, %s, line %d)\n", #cond, name, uplo ? "upper" : "lower", __LINE__); \
            return 1;                                                                                \
        }                                                                                            \
    } while (0)

static void to_csr(const matrix &m, std::vector<IndexType> &rp, std::vector<IndexType> &col, std::vector<ValueType> &val)
{
    rp.assign(1, 0);
    col.clear();
    val.clear();
    for (const auto &row : m) {
        for (const entry &e : row) {
            col.push_back(e.c);
            val.push_back(e.v);
        }
        rp.push_back((IndexType)col.size());
    }
}

static matrix reversed(const matrix &m)
{
    const IndexType n = (IndexType)m.size();
    matrix r(n);
    for (IndexType i = 0; i < n; ++i)
        for (const entry &e : m[i])
            r[n - 1 - i].push_back(entry{e.c < n ? n - 1 - e.c : e.c, e.v});
    return r;
}

// Everything the planner promises, on one matrix and one triangle. widths: the expected rows per
// level (empty: not checked). Returns 0 when all holds.
static int check(const char *name, const matrix &m, int uplo, int diag, const std::vector<uint32_t> &widths)
{
    const IndexType n = (IndexType)m.size();
    std::vector<IndexType> rp, col;
    std::vector<ValueType> val;
    to_csr(m, rp, col, val);
    trsv_plan p;
    plan_trsv(n, rp.data(), col.data(), uplo, diag, p);
    CHECK(p.bad_col_row == -1 && p.missing_diag_row == -1);
    auto dep = [&](IndexType r, IndexType c) { return uplo == SPMV_TRSV_LOWER ? c < r : c > r; };
    // the levels by relaxation to a fixed point, in no particular row order
    std::vector<uint32_t> ref(n, 0);
    for (bool changed = true; changed;) {
        changed = false;
        for (IndexType r = 0; r < n; ++r)
            for (const entry &e : m[r])
                if (dep(r, e.c) && ref[r] < ref[e.c] + 1) {
                    ref[r] = ref[e.c] + 1;
                    changed = true;
                }
    }
    CHECK(p.level.size() == n && p.offdiag.size() == n);
    uint64_t tri = 0;
    for (IndexType r = 0; r < n; ++r) {
        CHECK(p.level[r] == ref[r]);
        uint32_t off = 0;
        for (const entry &e : m[r]) {
            if (dep(r, e.c)) {
                CHECK(p.level[e.c] < p.level[r]);  // every dependency lies in a strictly lower level
                ++off;
            }
            tri += dep(r, e.c) || (e.c == r && diag == SPMV_TRSV_DIAG_NONUNIT);
        }
        CHECK(p.offdiag[r] == off);
    }
    CHECK(p.tri_nnz == tri);
    const uint32_t nlev = p.levels();
    CHECK(n == 0 ? nlev == 0 : nlev == *std::max_element(ref.begin(), ref.end()) + 1);
    CHECK(p.level_ptr.size() == size_t(nlev) + 1 && p.level_ptr[0] == 0 && p.level_ptr[nlev] == n);
    CHECK(p.long_ptr.size() == nlev && p.perm.size() == n && p.order.size() == n);
    // perm: a permutation sorted by (level, row), a level's rows contiguous
    std::vector<char> seen(n, 0);
    for (IndexType k = 0; k < n; ++k) {
        CHECK(p.perm[k] < n && !seen[p.perm[k]]);
        seen[p.perm[k]] = 1;
        if (k)
            CHECK(std::make_pair(p.level[p.perm[k - 1]], p.perm[k - 1]) < std::make_pair(p.level[p.perm[k]], p.perm[k]));
    }
    uint64_t widest = 0;
    for (uint32_t l = 0; l < nlev; ++l) {
        CHECK(p.level_ptr[l] < p.level_ptr[l + 1]);  // no empty level
        widest = std::max<uint64_t>(widest, p.level_ptr[l + 1] - p.level_ptr[l]);
        for (uint32_t k = p.level_ptr[l]; k < p.level_ptr[l + 1]; ++k)
            CHECK(p.level[p.perm[k]] == l);
        // the short and the long list partition the level: each ascending, split by the entry count
        CHECK(p.level_ptr[l] <= p.long_ptr[l] && p.long_ptr[l] <= p.level_ptr[l + 1]);
        std::vector<uint32_t> both;
        for (uint32_t k = p.level_ptr[l]; k < p.level_ptr[l + 1]; ++k) {
            const uint32_t r = p.order[k];
            CHECK(r < n && p.level[r] == l);
            const bool is_long = k >= p.long_ptr[l];
            CHECK((p.offdiag[r] > kTrsvLongRow) == is_long);
            if (k > p.level_ptr[l] && k != p.long_ptr[l])
                CHECK(p.order[k - 1] < r);
            both.push_back(r);
        }
        std::sort(both.begin(), both.end());
        CHECK(std::equal(both.begin(), both.end(), p.perm.begin() + p.level_ptr[l]));
    }
    CHECK(p.max_level_rows == widest);
    if (!widths.empty()) {
        CHECK(widths.size() == nlev);
        for (uint32_t l = 0; l < nlev; ++l)
            CHECK(p.level_ptr[l + 1] - p.level_ptr[l] == widths[l]);
    }
    // the launch list: every level once and in order; chains hold narrow levels only, and whole runs
    auto narrow = [&](uint32_t l) { return p.level_ptr[l + 1] - p.level_ptr[l] <= kTrsvChainRows; };
    uint32_t next = 0;
    uint64_t chain_levels = 0;
    for (size_t q = 0; q < p.launches.size(); ++q) {
        const trsv_launch &L = p.launches[q];
        CHECK(L.level_begin == next && L.level_end > L.level_begin && L.level_end <= nlev);
        if (L.chain) {
            for (uint32_t l = L.level_begin; l < L.level_end; ++l)
                CHECK(narrow(l));
            CHECK(L.level_begin == 0 || !narrow(L.level_begin - 1));  // the run is maximal (no cap on
            CHECK(L.level_end == nlev || !narrow(L.level_end));       // the levels of a launch)
            chain_levels += L.level_end - L.level_begin;
        } else {
            CHECK(L.level_end == L.level_begin + 1 && !narrow(L.level_begin));
        }
        next = L.level_end;
    }
    CHECK(next == nlev && p.nr_chain_levels == chain_levels);
    // the layout: every position's off-diagonal entries in CSR order, the diagonal summed in CSR order
    trsv_layout lay;
    build_trsv_layout(n, rp.data(), col.data(), val.data(), uplo, diag, p, lay);
    CHECK(lay.rp.size() == size_t(n) + 1 && lay.diag.size() == n && lay.col.size() == lay.rp[n] &&
          lay.val.size() == lay.rp[n]);
    for (IndexType k = 0; k < n; ++k) {
        const IndexType r = p.order[k];
        uint32_t w = lay.rp[k];
        ValueType d = diag == SPMV_TRSV_DIAG_UNIT ? 1 : 0;
        for (const entry &e : m[r]) {
            if (dep(r, e.c)) {
                CHECK(w < lay.rp[k + 1] && lay.col[w] == e.c && lay.val[w] == e.v);
                ++w;
            } else if (e.c == r && diag == SPMV_TRSV_DIAG_NONUNIT) {
                d += e.v;
            }
        }
        CHECK(w == lay.rp[k + 1] && lay.diag[k] == d);
    }
    // a substitution over the layout in position order solves the triangle (b = 1)
    std::vector<ValueType> x(n, NAN);
    for (IndexType k = 0; k < n; ++k) {
        ValueType s = 0;
        for (uint32_t e = lay.rp[k]; e < lay.rp[k + 1]; ++e)
            s += lay.val[e] * x[lay.col[e]];
        x[p.order[k]] = (1 - s) / lay.diag[k];
    }
    for (IndexType r = 0; r < n; ++r) {
        ValueType t = diag == SPMV_TRSV_DIAG_UNIT ? x[r] : 0, mag = 1;
        for (const entry &e : m[r])
            if (dep(r, e.c) || (e.c == r && diag == SPMV_TRSV_DIAG_NONUNIT)) {
                t += e.v * x[e.c];
                mag += std::fabs(e.v * x[e.c]);
            }
        CHECK(std::isfinite(x[r]) && std::fabs(t - 1) <= 1e-12 * mag);
    }
    return 0;
}

// the matrix as a LOWER problem and its reversal as an UPPER one
static int both(const char *name, const matrix &m, int diag, const std::vector<uint32_t> &widths)
{
    return check(name, m, SPMV_TRSV_LOWER, diag, widths) || check(name, reversed(m), SPMV_TRSV_UPPER, diag, widths);
}

// g x g 5-point grid, both triangles stored, diagonally dominant; unknown (i, j) has index id(i, j)
template <typename F>
static matrix grid(uint32_t g, F id)
{
    matrix m(size_t(g) * g);
    for (uint32_t i = 0; i < g; ++i)
        for (uint32_t j = 0; j < g; ++j) {
            auto &row = m[id(i, j)];
            if (i)
                row.push_back(entry{id(i - 1, j), -1});
            if (j)
                row.push_back(entry{id(i, j - 1), -1});
            row.push_back(entry{id(i, j), 5});
            if (j + 1 < g)
                row.push_back(entry{id(i, j + 1), -1});
            if (i + 1 < g)
                row.push_back(entry{id(i + 1, j), -1});
        }
    return m;
}

// level l holds widths[l] rows; every row past level 0 depends on `deps` rows of the level before
static matrix stacked(const std::vector<uint32_t> &widths, uint32_t deps)
{
    matrix m;
    IndexType prev = 0, prev_n = 0;
    for (uint32_t w : widths) {
        const IndexType first = (IndexType)m.size();
        for (uint32_t k = 0; k < w; ++k) {
            std::vector<entry> row;
            for (uint32_t d = 0; d < deps && prev_n; ++d)
                row.push_back(entry{prev + (k + d) % prev_n, ValueType(-0.25)});
            row.push_back(entry{first + k, ValueType(1 + deps)});
            m.push_back(row);
        }
        prev = first;
        prev_n = w;
    }
    return m;
}

int main()
{
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    const uint32_t cut = kTrsvChainRows, lcut = kTrsvLongRow;
    int rc = 0;
    rc |= both("n = 0", matrix(), SPMV_TRSV_DIAG_NONUNIT, {});
    rc |= both("n = 1", matrix{{entry{0, 2}}}, SPMV_TRSV_DIAG_NONUNIT, {1});
    {
        matrix m(300);
        for (IndexType r = 0; r < 300; ++r)
            m[r].push_back(entry{r, ValueType(1 + r)});
        rc |= both("diagonal", m, SPMV_TRSV_DIAG_NONUNIT, {300});
    }
    {
        const IndexType n = 1500;  // n levels of one row: one chain launch
        matrix m(n);
        for (IndexType r = 0; r < n; ++r) {
            if (r)
                m[r].push_back(entry{r - 1, -1});
            m[r].push_back(entry{r, 2});
        }
        rc |= both("bidiagonal chain", m, SPMV_TRSV_DIAG_NONUNIT, std::vector<uint32_t>(n, 1));
    }
    {
        const uint32_t g = 37;  // anti-diagonals: 2g - 1 levels of widths 1..g..1
        std::vector<uint32_t> w;
        for (uint32_t l = 0; l < 2 * g - 1; ++l)
            w.push_back(l < g ? l + 1 : 2 * g - 1 - l);
        const matrix nat = grid(g, [g](uint32_t i, uint32_t j) { return i * g + j; });
        rc |= check("grid, natural order", nat, SPMV_TRSV_LOWER, SPMV_TRSV_DIAG_NONUNIT, w);
        rc |= check("grid, natural order", nat, SPMV_TRSV_UPPER, SPMV_TRSV_DIAG_NONUNIT, w);
        // red-black order: the (g * g + 1) / 2 red unknowns (i + j even) first
        const uint32_t nred = (g * g + 1) / 2;
        const matrix rb = grid(g, [g, nred](uint32_t i, uint32_t j) {
            const uint32_t k = i * g + j;  // g odd: the colours alternate along k
            return k % 2 == 0 ? k / 2 : nred + k / 2;
        });
        rc |= check("grid, red-black order", rb, SPMV_TRSV_LOWER, SPMV_TRSV_DIAG_NONUNIT, {nred, g * g - nred});
        rc |= check("grid, red-black order", rb, SPMV_TRSV_UPPER, SPMV_TRSV_DIAG_NONUNIT, {g * g - nred, nred});
        rc |= check("grid, unit diagonal", nat, SPMV_TRSV_LOWER, SPMV_TRSV_DIAG_UNIT, w);
    }
    {
        const IndexType n = 3000;  // random lower triangle, up to 6 entries per row at random columns < r
        matrix m(n);
        for (IndexType r = 0; r < n; ++r) {
            double sum = 0;
            for (int k = 0; k < 6 && r; ++k) {
                const double v = uni(rng);
                m[r].push_back(entry{IndexType(rng() % r), ValueType(v)});
                sum += std::fabs(v);
            }
            m[r].push_back(entry{r, ValueType(1 + sum)});
        }
        rc |= both("random lower triangle", m, SPMV_TRSV_DIAG_NONUNIT, {});
    }
    {
        const IndexType n = 400;  // arrow: the last row dense (a long row in a level of its own)
        matrix m(n);
        for (IndexType r = 0; r + 1 < n; ++r)
            m[r].push_back(entry{r, 2});
        for (IndexType c = 0; c + 1 < n; ++c)
            m[n - 1].push_back(entry{c, ValueType(0.5)});
        m[n - 1].push_back(entry{n - 1, ValueType(n)});
        rc |= both("arrow", m, SPMV_TRSV_DIAG_NONUNIT, {n - 1, 1});
    }
    // level widths around the chain cut: a chain of two levels, a wide launch, a chain of one, a wide launch
    rc |= both("widths straddling the chain cut", stacked({cut - 1, cut, cut + 1, 1, cut + 1}, 2),
               SPMV_TRSV_DIAG_NONUNIT, {cut - 1, cut, cut + 1, 1, cut + 1});
    {
        trsv_plan p;
        std::vector<IndexType> rp, col;
        std::vector<ValueType> val;
        to_csr(stacked({cut - 1, cut, cut + 1, 1, cut + 1}, 2), rp, col, val);
        plan_trsv((IndexType)rp.size() - 1, rp.data(), col.data(), SPMV_TRSV_LOWER, SPMV_TRSV_DIAG_NONUNIT, p);
        const trsv_launch want[4] = {{1, 0, 2}, {0, 2, 3}, {1, 3, 4}, {0, 4, 5}};
        bool same = p.launches.size() == 4;
        for (size_t q = 0; same && q < 4; ++q)
            same = p.launches[q].chain == want[q].chain && p.launches[q].level_begin == want[q].level_begin &&
                   p.launches[q].level_end == want[q].level_end;
        if (!same) {
            std::fprintf(stderr, "FAILED launch list of the straddling widths\n");
            rc = 1;
        }
    }
    // row lengths around the long-row cut, in a narrow and in a wide level
    rc |= both("rows at the long cut, narrow level", stacked({200, 64}, lcut), SPMV_TRSV_DIAG_NONUNIT, {200, 64});
    rc |= both("rows past the long cut, narrow level", stacked({200, 64}, lcut + 1), SPMV_TRSV_DIAG_NONUNIT, {200, 64});
    rc |= both("rows past the long cut, wide level", stacked({200, cut + 3}, lcut + 1), SPMV_TRSV_DIAG_NONUNIT,
               {200, cut + 3});
    {
        // unsorted columns, duplicate off-diagonal and duplicate diagonal entries, entries of the other triangle
        const IndexType n = 500;
        matrix m(n);
        for (IndexType r = 0; r < n; ++r) {
            m[r].push_back(entry{r, 3});
            if (r + 1 < n)
                m[r].push_back(entry{r + 1, ValueType(0.5)});
            if (r >= 2) {
                m[r].push_back(entry{r - 1, ValueType(-0.5)});
                m[r].push_back(entry{r - 2, ValueType(0.25)});
                m[r].push_back(entry{r - 1, ValueType(-0.125)});
            }
            m[r].push_back(entry{r, 1});
        }
        rc |= both("unsorted columns and duplicates", m, SPMV_TRSV_DIAG_NONUNIT, {});
        rc |= both("unsorted columns and duplicates, unit", m, SPMV_TRSV_DIAG_UNIT, {});
    }
    {
        // rows 7 and 11 have no stored diagonal: refused under NONUNIT naming row 7 (the mirrored
        // rows under UPPER), accepted under UNIT
        const IndexType n = 20;
        matrix m(n);
        for (IndexType r = 0; r < n; ++r) {
            if (r)
                m[r].push_back(entry{r - 1, ValueType(0.5)});
            if (r != 7 && r != 11)
                m[r].push_back(entry{r, 2});
        }
        for (int uplo : {SPMV_TRSV_LOWER, SPMV_TRSV_UPPER}) {
            const matrix &mm = uplo == SPMV_TRSV_LOWER ? m : reversed(m);
            std::vector<IndexType> rp, col;
            std::vector<ValueType> val;
            to_csr(mm, rp, col, val);
            trsv_plan p;
            plan_trsv(n, rp.data(), col.data(), uplo, SPMV_TRSV_DIAG_NONUNIT, p);
            const int64_t want = uplo == SPMV_TRSV_LOWER ? 7 : n - 1 - 11;
            if (p.missing_diag_row != want || p.bad_col_row != -1) {
                std::fprintf(stderr, "FAILED missing diagonal: row %lld, expected %lld\n", (long long)p.missing_diag_row,
                             (long long)want);
                rc = 1;
            }
            rc |= check("missing diagonal under unit", mm, uplo, SPMV_TRSV_DIAG_UNIT, {});
            // a column index >= n names its row, wherever the entry lies
            col[rp[5]] = n + 3;
            plan_trsv(n, rp.data(), col.data(), uplo, SPMV_TRSV_DIAG_UNIT, p);
            if (p.bad_col_row != 5) {
                std::fprintf(stderr, "FAILED column out of range: row %lld\n", (long long)p.bad_col_row);
                rc = 1;
            }
        }
    }
    if (rc)
        return 1;
    std::printf("OK trsv plan\n");
    return 0;
}
