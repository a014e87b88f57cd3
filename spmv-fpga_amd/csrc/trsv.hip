// Sparse triangular solve by level scheduling (include/csr_hw_wrapper.h Part 5).
//
// The host planner (trsv_plan.cpp) sorts the rows by dependency level; this file uploads the layout
// and walks the launch list. Device layout, over the positions p of trsv_plan::order:
//   rp    u32[n + 1]  off-diagonal entries of position p: [rp[p], rp[p + 1])
//   col   u32[]       their matrix columns (indices into x), CSR order inside a row
//   val   V[]         their values
//   diag  V[n]        the diagonal of position p
//   rows  u32[n]      the matrix row of position p (where b is read and x written)
//   level_ptr u32[levels + 1], long_ptr u32[levels]: positions [level_ptr[l], long_ptr[l]) are level
//                     l's short rows (a thread each), [long_ptr[l], level_ptr[l + 1]) its long rows
//                     (more than kTrsvLongRow entries: a wave each)
// Ordering. The kernel boundary is the only ordering between workgroups: k_trsv_level reads only x
// values that earlier launches wrote, and k_trsv_chain is ONE workgroup. No workgroup ever waits
// for another inside a launch (no flags, no spinning, no grid sync), so a solve cannot hang on
// forward progress or on the visibility of plain stores between compute units.
// Determinism. A short row adds its products in CSR order; a long row's lane k adds entries k,
// k + 64, ... in order and the 64 partial sums meet in a fixed shuffle tree. No atomics.
// b and x carry no __restrict__: they may be the same array (the thread or wave that reads b_i is
// the one that writes x_i), and the chain kernel reads back x values it has written.
#include <algorithm>
#include <cstring>
#include <memory>

#include "spmv_internal.hpp"

struct spmv_trsv {
    int device = 0, uplo = 0, diag = 0;
    IndexType n = 0;
    uint64_t tri_nnz = 0, levels = 0, chain_levels = 0, max_level_rows = 0, bytes = 0;
    std::vector<spmvhw::trsv_launch> launches;
    std::vector<uint32_t> level_ptr, long_ptr;  // host copies: the wide launches' arguments
    uint32_t *d_rp = nullptr, *d_col = nullptr, *d_rows = nullptr, *d_level_ptr = nullptr, *d_long_ptr = nullptr;
    ValueType *d_val = nullptr, *d_diag = nullptr;
    ~spmv_trsv()
    {
        if (!d_rp && !d_rows)
            return;  // an empty handle never touched the device
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        for (void *p : {(void *)d_rp, (void *)d_col, (void *)d_rows, (void *)d_level_ptr, (void *)d_long_ptr,
                        (void *)d_val, (void *)d_diag})
            if (p)
                (void)hipFree(p);
    }
};

namespace spmvhw {

namespace {

constexpr int kTrsvLevelThreads = 256;  // wide level: 256 short rows or 4 long rows per workgroup
constexpr int kTrsvChainThreads = 1024;

struct trsv_dev {
    const uint32_t *__restrict__ rp;
    const uint32_t *__restrict__ col;
    const ValueType *__restrict__ val;
    const ValueType *__restrict__ diag;
    const uint32_t *__restrict__ rows;
};

// one thread solves position p: products added in CSR order
__device__ __forceinline__ void trsv_row_thread(const trsv_dev &L, uint64_t p, const ValueType *b, ValueType *x)
{
    ValueType s = 0;
    for (uint32_t e = L.rp[p], end = L.rp[p + 1]; e < end; ++e)
        s += L.val[e] * x[L.col[e]];
    const uint32_t r = L.rows[p];
    x[r] = (b[r] - s) / L.diag[p];
}

// one wave solves position p (all 64 lanes call it): a strided partial sum per lane, then a fixed tree
__device__ __forceinline__ void trsv_row_wave(const trsv_dev &L, uint64_t p, uint32_t lane, const ValueType *b,
                                              ValueType *x)
{
    ValueType s = 0;
    for (uint64_t e = uint64_t(L.rp[p]) + lane, end = L.rp[p + 1]; e < end; e += kWave)
        s += L.val[e] * x[L.col[e]];
    for (int off = kWave / 2; off > 0; off >>= 1)
        s += __shfl_down(s, off, kWave);
    if (lane == 0) {
        const uint32_t r = L.rows[p];
        x[r] = (b[r] - s) / L.diag[p];
    }
}

// One wide level: positions [begin, begin + nshort) a thread each in the first short_blocks
// workgroups, [begin + nshort, begin + nshort + nlong) a wave each in the others. Every x it reads
// was written by an earlier launch.
__global__ __launch_bounds__(kTrsvLevelThreads) void k_trsv_level(trsv_dev L, uint32_t begin, uint32_t nshort,
                                                                  uint32_t nlong, uint32_t short_blocks,
                                                                  const ValueType *b, ValueType *x)
{
    if (blockIdx.x < short_blocks) {
        const uint32_t k = blockIdx.x * kTrsvLevelThreads + threadIdx.x;
        if (k < nshort)
            trsv_row_thread(L, uint64_t(begin) + k, b, x);
    } else {
        const uint32_t w = (blockIdx.x - short_blocks) * (kTrsvLevelThreads / kWave) + threadIdx.x / kWave;
        if (w < nlong)  // wave-uniform
            trsv_row_wave(L, uint64_t(begin) + nshort + w, threadIdx.x % kWave, b, x);
    }
}

// A run of narrow levels [lb, le) in ONE workgroup, a barrier between levels. The x values a level
// writes are read by later levels of the same workgroup: its waves share one compute unit's vector
// L1 (the library is never built in threadgroup-split mode), which takes the unit's stores and
// loads in issue order, and __syncthreads() is the workgroup-scope release, the barrier and the
// workgroup-scope acquire in one (for gfx950 outside threadgroup-split mode the compiler's memory
// model needs no cache action for that scope), so after the barrier every wave's ordinary loads see
// them. No hand-rolled barrier, no flag. lb and le are launch arguments and the row loops end on
// wave-uniform bounds, so every thread reaches every barrier.
__global__ __launch_bounds__(kTrsvChainThreads) void k_trsv_chain(trsv_dev L,
                                                                  const uint32_t *__restrict__ level_ptr,
                                                                  const uint32_t *__restrict__ long_ptr, uint32_t lb,
                                                                  uint32_t le, const ValueType *b, ValueType *x)
{
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    for (uint32_t l = lb; l < le; ++l) {
        const uint64_t first = level_ptr[l], first_long = long_ptr[l], end = level_ptr[l + 1];
        for (uint64_t p = first + tid; p < first_long; p += kTrsvChainThreads)
            trsv_row_thread(L, p, b, x);
        for (uint64_t p = first_long + wave; p < end; p += kTrsvChainThreads / kWave)
            trsv_row_wave(L, p, lane, b, x);
        __syncthreads();
    }
}

trsv_dev dev_of(const spmv_trsv &t) { return trsv_dev{t.d_rp, t.d_col, t.d_val, t.d_diag, t.d_rows}; }

// the launch list on s; warm: only load the two kernels' code objects
hipError_t launch_trsv(const spmv_trsv &t, const ValueType *d_b, ValueType *d_x, hipStream_t s, bool warm)
{
    const trsv_dev L = dev_of(t);
    if (warm) {
        launch_or_warm(true, k_trsv_level, dim3(1), dim3(kTrsvLevelThreads), 0, s, L, 0u, 0u, 0u, 0u, d_b, d_x);
        launch_or_warm(true, k_trsv_chain, dim3(1), dim3(kTrsvChainThreads), 0, s, L, (const uint32_t *)nullptr,
                       (const uint32_t *)nullptr, 0u, 0u, d_b, d_x);
        return hipSuccess;
    }
    for (const trsv_launch &q : t.launches) {
        if (q.chain) {
            hipLaunchKernelGGL(k_trsv_chain, dim3(1), dim3(kTrsvChainThreads), 0, s, L,
                               (const uint32_t *)t.d_level_ptr, (const uint32_t *)t.d_long_ptr, q.level_begin,
                               q.level_end, d_b, d_x);
        } else {
            const uint32_t begin = t.level_ptr[q.level_begin], first_long = t.long_ptr[q.level_begin];
            const uint32_t nshort = first_long - begin, nlong = t.level_ptr[q.level_end] - first_long;
            const uint32_t sb = (nshort + kTrsvLevelThreads - 1) / kTrsvLevelThreads;
            const uint32_t per = kTrsvLevelThreads / kWave, lb = (nlong + per - 1) / per;
            hipLaunchKernelGGL(k_trsv_level, dim3(sb + lb), dim3(kTrsvLevelThreads), 0, s, L, begin, nshort, nlong, sb,
                               d_b, d_x);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

template <typename T>
int upload_array(T *&dst, const std::vector<T> &src, uint64_t &bytes, hipStream_t s)
{
    const size_t b = std::max<size_t>(src.size(), 1) * sizeof(T);
    SPMV_TRY(hipMalloc((void **)&dst, b));
    bytes += b;
    return src.empty() ? 0 : upload_staged(dst, src.data(), src.size() * sizeof(T), s);
}

bool bad_trsv_mode(const char *who, int uplo, int diag)
{
    if (uplo != SPMV_TRSV_LOWER && uplo != SPMV_TRSV_UPPER) {
        set_error(std::string(who) + ": uplo must be SPMV_TRSV_LOWER (0) or SPMV_TRSV_UPPER (1)");
        return true;
    }
    if (diag != SPMV_TRSV_DIAG_NONUNIT && diag != SPMV_TRSV_DIAG_UNIT) {
        set_error(std::string(who) + ": diag must be SPMV_TRSV_DIAG_NONUNIT (0) or SPMV_TRSV_DIAG_UNIT (1)");
        return true;
    }
    return false;
}

int trsv_create_from_slice(const char *who, spmv_trsv **out, int device, int uplo, int diag, const csr_slice &sl)
{
    if (sl.n != sl.m) {
        set_error(std::string(who) + ": the matrix must be square");
        return 1;
    }
    std::unique_ptr<spmv_trsv> t(new spmv_trsv);
    t->device = device;
    t->uplo = uplo;
    t->diag = diag;
    t->n = sl.n;
    if (sl.n == 0) {
        *out = t.release();
        return 0;
    }
    SPMV_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)sl.stream;
    const uint64_t nnz = sl.nnz();
    if (nnz && (!sl.col || !sl.val)) {
        set_error(std::string(who) + ": null argument");
        return 1;
    }
    // the analysis and the layout are host work: a device slice's entries come back once
    std::vector<IndexType> h_col;
    std::vector<ValueType> h_val;
    const IndexType *col = sl.col;
    const ValueType *val = sl.val;
    if (sl.on_device && nnz) {
        h_col.resize(nnz);
        h_val.resize(nnz);
        SPMV_TRY(hipMemcpyAsync(h_col.data(), sl.col, nnz * sizeof(IndexType), hipMemcpyDeviceToHost, s));
        SPMV_TRY(hipMemcpyAsync(h_val.data(), sl.val, nnz * sizeof(ValueType), hipMemcpyDeviceToHost, s));
        SPMV_TRY(hipStreamSynchronize(s));
        col = h_col.data();
        val = h_val.data();
    }
    trsv_plan plan;
    plan_trsv(sl.n, sl.rp.data(), col, uplo, diag, plan);
    if (plan.bad_col_row >= 0) {
        set_error(std::string(who) + ": column index out of range (>= n) in row " + std::to_string(plan.bad_col_row));
        return 1;
    }
    if (plan.missing_diag_row >= 0) {
        set_error(std::string(who) + ": missing diagonal in row " + std::to_string(plan.missing_diag_row));
        return 1;
    }
    trsv_layout lay;
    build_trsv_layout(sl.n, sl.rp.data(), col, val, uplo, diag, plan, lay);
    t->tri_nnz = plan.tri_nnz;
    t->levels = plan.levels();
    t->chain_levels = plan.nr_chain_levels;
    t->max_level_rows = plan.max_level_rows;
    if (upload_array(t->d_rp, lay.rp, t->bytes, s) || upload_array(t->d_col, lay.col, t->bytes, s) ||
        upload_array(t->d_val, lay.val, t->bytes, s) || upload_array(t->d_diag, lay.diag, t->bytes, s) ||
        upload_array(t->d_rows, plan.order, t->bytes, s) || upload_array(t->d_level_ptr, plan.level_ptr, t->bytes, s) ||
        upload_array(t->d_long_ptr, plan.long_ptr, t->bytes, s))
        return 1;
    t->launches = std::move(plan.launches);
    t->level_ptr = std::move(plan.level_ptr);
    t->long_ptr = std::move(plan.long_ptr);
    (void)launch_trsv(*t, nullptr, nullptr, s, true);
    *out = t.release();
    return 0;
}

}  // namespace

}  // namespace spmvhw

using namespace spmvhw;

extern "C" {

int spmv_trsv_create_device(spmv_trsv **t, int device, int uplo, int diag, IndexType n, IndexType nr_nzeros,
                            const IndexType *d_row_ptr, const IndexType *d_col_ind, const ValueType *d_values,
                            void *stream)
{
    const char *who = "spmv_trsv_create_device";
    if (bad_trsv_mode(who, uplo, diag) || slice_device_args(who, t, n, d_row_ptr))
        return 1;
    csr_slice sl;
    if (n == 0) {  // an empty handle needs no device
        sl.rp.assign(1, 0u);
        return trsv_create_from_slice(who, t, device, uplo, diag, sl);
    }
    if (slice_from_device(who, sl, t, device, n, n, nr_nzeros, d_row_ptr, d_col_ind, d_values, (hipStream_t)stream))
        return 1;
    return trsv_create_from_slice(who, t, device, uplo, diag, sl);
}

int spmv_trsv_create_host(spmv_trsv **t, int device, int uplo, int diag, const csr_matrix *matrix)
{
    const char *who = "spmv_trsv_create_host";
    csr_slice sl;
    if (bad_trsv_mode(who, uplo, diag) || slice_from_host(who, sl, t, matrix, 0, matrix ? matrix->nr_rows : 0))
        return 1;
    return trsv_create_from_slice(who, t, device, uplo, diag, sl);
}

int spmv_trsv_solve(const spmv_trsv *t, const ValueType *d_b, ValueType *d_x, void *stream)
{
    if (!t) {
        set_error("spmv_trsv_solve: null handle");
        return 1;
    }
    if (t->n == 0)
        return 0;
    if (!d_b || !d_x) {
        set_error("spmv_trsv_solve: null argument");
        return 1;
    }
    SPMV_TRY(hipSetDevice(t->device));
    SPMV_TRY(launch_trsv(*t, d_b, d_x, (hipStream_t)stream, false));
    return 0;
}

int spmv_trsv_get_stats(const spmv_trsv *t, spmv_trsv_stats *st)
{
    if (!t || !st) {
        set_error("spmv_trsv_get_stats: null argument");
        return 1;
    }
    std::memset(st, 0, sizeof(*st));
    st->n = t->n;
    st->nr_nzeros = t->tri_nnz;
    st->nr_levels = t->levels;
    st->nr_launches = t->launches.size();
    st->nr_chain_levels = t->chain_levels;
    st->max_level_rows = t->max_level_rows;
    st->device_bytes = t->bytes;
    st->device = t->device;
    st->uplo = t->uplo;
    st->diag = t->diag;
    return 0;
}

void spmv_trsv_destroy(spmv_trsv *t) { delete t; }

}  // extern "C"
