// Host planner of the sparse triangular solve (spmv_trsv_*): level analysis, launch
// list and permuted layout. Pure functions of their arguments, no HIP and no environment;
// tests/trsv_host compiles this file alone with g++ -fsanitize=address,undefined.
#include <algorithm>

#include "spmv_host.hpp"

namespace spmvhw {

namespace {
// entry (r, c) belongs to the triangle's off-diagonal part
inline bool in_triangle(int uplo, IndexType r, IndexType c) { return uplo == SPMV_TRSV_LOWER ? c < r : c > r; }
}  // namespace

void plan_trsv(IndexType n, const IndexType *rp, const IndexType *col, int uplo, int diag, trsv_plan &out)
{
    out = trsv_plan();
    out.level.assign(n, 0);
    out.offdiag.assign(n, 0);
    uint32_t nlev = 0;
    for (IndexType k = 0; k < n; ++k) {
        const IndexType r = uplo == SPMV_TRSV_LOWER ? k : n - 1 - k;
        uint32_t lvl = 0, off = 0;
        bool has_diag = false;
        for (IndexType e = rp[r]; e < rp[r + 1]; ++e) {
            const IndexType c = col[e];
            if (c >= n) {
                if (out.bad_col_row < 0 || r < out.bad_col_row)
                    out.bad_col_row = r;
                continue;
            }
            if (c == r) {
                has_diag = true;
                out.tri_nnz += diag == SPMV_TRSV_DIAG_UNIT ? 0 : 1;
            } else if (in_triangle(uplo, r, c)) {  // its row came earlier in this pass: level[c] is final
                lvl = std::max(lvl, out.level[c] + 1);
                ++off;
            }
        }
        if (!has_diag && diag != SPMV_TRSV_DIAG_UNIT && (out.missing_diag_row < 0 || r < out.missing_diag_row))
            out.missing_diag_row = r;
        out.level[r] = lvl;
        out.offdiag[r] = off;
        out.tri_nnz += off;
        nlev = std::max(nlev, lvl + 1);
    }
    if (n == 0)
        nlev = 0;
    // counting sort by level, the rows of a level in index order
    out.level_ptr.assign(size_t(nlev) + 1, 0);
    std::vector<uint32_t> nlong(nlev, 0);
    for (IndexType r = 0; r < n; ++r) {
        ++out.level_ptr[out.level[r] + 1];
        nlong[out.level[r]] += out.offdiag[r] > kTrsvLongRow;
    }
    for (uint32_t l = 0; l < nlev; ++l)
        out.level_ptr[l + 1] += out.level_ptr[l];
    out.perm.assign(n, 0);
    out.order.assign(n, 0);
    out.long_ptr.assign(nlev, 0);
    std::vector<uint32_t> at(nlev), at_short(nlev), at_long(nlev);
    for (uint32_t l = 0; l < nlev; ++l) {
        out.long_ptr[l] = out.level_ptr[l + 1] - nlong[l];
        at[l] = at_short[l] = out.level_ptr[l];
        at_long[l] = out.long_ptr[l];
        out.max_level_rows = std::max<uint64_t>(out.max_level_rows, out.level_ptr[l + 1] - out.level_ptr[l]);
    }
    for (IndexType r = 0; r < n; ++r) {
        const uint32_t l = out.level[r];
        out.perm[at[l]++] = r;
        out.order[(out.offdiag[r] > kTrsvLongRow ? at_long[l] : at_short[l])++] = r;
    }
    // the launch list: every maximal run of narrow levels is one chain launch, any other level a wide one
    for (uint32_t l = 0; l < nlev;) {
        auto narrow = [&](uint32_t q) { return out.level_ptr[q + 1] - out.level_ptr[q] <= kTrsvChainRows; };
        uint32_t e = l + 1;
        if (narrow(l)) {
            while (e < nlev && narrow(e))
                ++e;
            out.nr_chain_levels += e - l;
        }
        out.launches.push_back(trsv_launch{narrow(l) ? 1u : 0u, l, e});
        l = e;
    }
}

void build_trsv_layout(IndexType n, const IndexType *rp, const IndexType *col, const ValueType *val, int uplo,
                       int diag, const trsv_plan &plan, trsv_layout &out)
{
    out = trsv_layout();
    out.rp.assign(size_t(n) + 1, 0);
    for (IndexType p = 0; p < n; ++p)
        out.rp[p + 1] = out.rp[p] + plan.offdiag[plan.order[p]];
    out.col.resize(out.rp[n]);
    out.val.resize(out.rp[n]);
    out.diag.assign(n, ValueType(diag == SPMV_TRSV_DIAG_UNIT ? 1 : 0));
    for (IndexType p = 0; p < n; ++p) {
        const IndexType r = plan.order[p];
        uint32_t w = out.rp[p];
        for (IndexType e = rp[r]; e < rp[r + 1]; ++e) {
            const IndexType c = col[e];
            if (c == r) {
                if (diag != SPMV_TRSV_DIAG_UNIT)
                    out.diag[p] += val[e];
            } else if (c < n && in_triangle(uplo, r, c)) {
                out.col[w] = c;
                out.val[w] = val[e];
                ++w;
            }
        }
    }
}

}  // namespace spmvhw
