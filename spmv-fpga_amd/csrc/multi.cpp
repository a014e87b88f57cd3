// spmv_multi: Y = A * X for 1..8 right-hand sides per call (include/csr_hw_wrapper.h Part 2).
//
// Native paths, for 2, 4 or 8 vectors: the slice plan's one-pass kernel (slices.hip,
// k_spmv_slices_multi; banded and stencil-like matrices) and the panel sweep with nvec
// accumulators per row (sweep_multi.hip, k_spmv_sweep_multi; scattered matrices
// from 1M rows). Fallback, for every other kernel and vector count: an ordinary plan,
// X split into contiguous vectors, one plan run per vector, the results interleaved into Y.
// The reference multiplies by one vector per call (spmv.cpp:280-294 copies one x per CU).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "spmv_internal.hpp"

using namespace spmvhw;

struct spmv_multi {
    spmv_plan *plan = nullptr;
    int nvec = 1;
    bool native = false;
    ValueType *d_xs = nullptr;  // fallback: nvec contiguous vectors of nr_cols
    ValueType *d_ys = nullptr;  // fallback: nvec contiguous results of nr_rows
    ~spmv_multi()
    {
        if (plan) {
            (void)hipSetDevice(plan->device);
            (void)hipDeviceSynchronize();
        }
        if (d_xs)
            (void)hipFree(d_xs);
        if (d_ys)
            (void)hipFree(d_ys);
        delete plan;
    }
};

namespace spmvhw {

// The automatic choice's padding limit: the native path is taken while 64 * slots <= limit * nnz.
// Each limit is the highest padding at which the native path beat the fallback by more than the
// two measurements' spread on the power-law generator (500k rows, 16 per row, rows capped so
// that the padding is 1.25 .. 6; tools/multi_bench.py --crossover, profiles/multi_bench.jsonl
// tag "crossover"). fp64, fallback on the sweep: nvec 2 wins at 1.5 (0.087 vs
// 0.093 ms) and ties at 1.75; nvec 4 wins at 4.0 (0.170 vs 0.178) and loses at 5.0; nvec 8 wins
// at 6.0 (0.279 vs 0.350). fp32, fallback on the tiles: nvec 2 wins at 3.0 (0.080 vs 0.095) and
// is within 2 % at 4.0; nvec 4 (0.160 vs 0.184) and nvec 8 (0.217 vs 0.361) win at 6.0, the last padding
// measured with capped rows.
static double multi_pad_limit(int nvec)
{
    if (sizeof(ValueType) == 8)
        return nvec == 2 ? 1.5 : nvec == 4 ? 4.0 : 6.0;
    return nvec == 2 ? 3.0 : 6.0;
}

// dst[j * n + i] = src[i * K + j]: X (row-major, K per row) into K contiguous vectors. A wave
// reads 64 consecutive values and writes K runs of 64 / K.
__global__ void k_multi_split(const ValueType *__restrict__ src, ValueType *__restrict__ dst, uint64_t n, uint32_t K)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * K)
        dst[(t % K) * n + t / K] = src[t];
}

// dst[i * K + j] = src[j * n + i]: K contiguous results into Y (row-major)
__global__ void k_multi_join(const ValueType *__restrict__ src, ValueType *__restrict__ dst, uint64_t n, uint32_t K)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * K)
        dst[t] = src[(t % K) * n + t / K];
}

static bool multi_native_nvec(int nvec) { return nvec == 2 || nvec == 4 || nvec == 8; }

// The automatic choice of the one-pass sweep (sweep_multi.hip): the fewest rows from which a
// scattered matrix (one whose single-vector automatic kernel is the sweep or binned) takes it at
// this nvec; 0: never. No switch forces the path (the library reads only the environment switches
// INTEGRATION.md lists). plan_create_from_slice adds the condition that the unsplit panels fill a
// round of workgroups (from 2.61M / 1.30M / 0.65M rows for nvec 2 / 4 / 8 on 256 CUs).
// Measured on the power-law generator, 16 per row, at 1M, 3M and 10M rows, the sweep where this
// rule takes it against the fallback on the matrix's automatic kernel, alternating in one process
// (tools/multi_bench.py --scattered, profiles/multi_bench.jsonl tag "scattered"),
// ms native / fallback. fp64 (fallback on the sweep): nvec 2 at 3M, 10M 0.357 / 0.430, 1.330 /
// 1.683; nvec 4 0.494 / 0.879, 2.163 / 3.356; nvec 8 at 1M, 3M, 10M 0.221 / 0.584, 0.798 / 1.756,
// 3.083 / 6.647. fp32 (fallback on the sweep, at 10M on binned): nvec 4 at 3M, 10M 0.373 / 0.646,
// 1.817 / 2.036; nvec 8 0.199 / 0.497, 0.749 / 1.338, 2.735 / 4.097. Every win is at least four
// times the sum of the two min-max spreads. 1M is the smallest size measured. fp32 nvec 2 has no
// measured win to show (the tool cannot time a path this rule declines; its fallback at 10M rows
// is the binned kernel, 1.03 ms, which nvec 4 beats by only 1.12x), so it stays off.
static uint64_t multi_sweep_min_rows(int nvec)
{
    if (sizeof(ValueType) == 4 && nvec == 2)
        return 0;
    return 1000000;
}

// 64-row slices' stored entries (64 * slots) from row_ptr alone, as build_slices counts them
static uint64_t slice_stored_entries(const IndexType *rp, IndexType n)
{
    uint64_t slots = 0;
    for (uint64_t q = 0; q < n; q += kWave) {
        uint32_t L = 0;
        for (uint64_t r = q; r < std::min<uint64_t>(n, q + kWave); ++r)
            L = std::max<uint32_t>(L, rp[r + 1] - rp[r]);
        slots += L;
    }
    return slots * kWave;
}

// Decides the path, builds the plan and the fallback's scratch. op = SPMV_OP_T: the slice's
// transpose (transpose.hip), then the same decision and build on A^T.
static int multi_create(spmv_multi **out, int device, int op, const csr_slice &sl, int nvec)
{
    if (op == SPMV_OP_T) {
        SPMV_TRY(hipSetDevice(device));
        transposed_csr t;
        if (transpose_slice(t, sl) || multi_create(out, device, SPMV_OP_N, t.slice, nvec))
            return 1;
        (*out)->plan->op = SPMV_OP_T;
        return 0;
    }
    const IndexType nr_rows = sl.n, nr_cols = sl.m;
    hipStream_t s = (hipStream_t)sl.stream;
    const int requested = requested_kernel();  // env SPMV_HW_KERNEL
    bool native = false;
    int sweep_nvec = 1;  // > 1: plan_create_from_slice may build the multi-vector sweep
    if (multi_native_nvec(nvec)) {
        if (requested == kKernelSlices) {
            native = true;
        } else if (requested == -1 && nr_rows) {
            const uint64_t nnz = sl.nnz(), stored = slice_stored_entries(sl.rp.data(), nr_rows);
            native = nnz > 0 && stored <= 0xFFFFFFFFull && double(stored) <= multi_pad_limit(nvec) * double(nnz);
            // the slice rule declines: a candidate for the sweep (plan_create_from_slice decides
            // on the matrix's automatic kernel and the panel count). SPMV_SWEEP_DETERMINISTIC=1
            // asks for fixed bits, which the fallback on the turn-ordered sweep gives
            const char *det = std::getenv("SPMV_SWEEP_DETERMINISTIC");
            const uint64_t min_rows = multi_sweep_min_rows(nvec);
            if (!native && min_rows && nr_rows >= min_rows && !(det && det[0] == '1'))
                sweep_nvec = nvec;
        }
    }
    std::unique_ptr<spmv_multi> m(new spmv_multi());
    m->nvec = nvec;
    if (plan_create_from_slice(&m->plan, device, SPMV_OP_N, sl, native ? kKernelSlices : -1, sweep_nvec))
        return 1;
    if (native && m->plan->kernel != kKernelSlices) {
        set_error("spmv_multi: internal: the native path needs a slice plan");
        return 1;
    }
    native = native || m->plan->sweep.nvec > 1;  // the automatic choice took the sweep
    m->native = native;
    if (native) {
        // load the code object (a sweep plan's build has warmed launch_sweep_multi)
        if (m->plan->kernel == kKernelSlices)
            (void)launch_slices_multi(*m->plan, nvec, nullptr, nullptr, s, true);
        (void)hipGetLastError();
    } else if (nvec > 1) {
        SPMV_TRY(hipMalloc((void **)&m->d_xs, std::max<uint64_t>(uint64_t(nr_cols) * nvec, 1) * sizeof(ValueType)));
        SPMV_TRY(hipMalloc((void **)&m->d_ys, std::max<uint64_t>(uint64_t(nr_rows) * nvec, 1) * sizeof(ValueType)));
        launch_or_warm(true, k_multi_split, dim3(1), dim3(256), 0, s, (const ValueType *)nullptr, (ValueType *)nullptr,
                       uint64_t(0), 0u);
        launch_or_warm(true, k_multi_join, dim3(1), dim3(256), 0, s, (const ValueType *)nullptr, (ValueType *)nullptr,
                       uint64_t(0), 0u);
        (void)hipGetLastError();
    }
    *out = m.release();
    return 0;
}

static bool multi_bad_nvec(const char *who, int nvec)
{
    if (nvec >= 1 && nvec <= 8)
        return false;
    set_error(std::string(who) + ": nvec must be 1..8");
    return true;
}

// The four multi creates: `who` names the caller in the messages (op = SPMV_OP_N through an _op
// function is the function without an op, and reports as it). nvec is checked after the other
// arguments and before the first HIP call, which slice_from_device makes.
static int create_device(const char *who, spmv_multi **m, int device, int op, IndexType nr_rows, IndexType nr_cols,
                         IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col_ind,
                         const ValueType *d_values, int nvec, void *stream)
{
    if (slice_device_args(who, m, nr_rows, d_row_ptr))
        return 1;
    *m = nullptr;
    csr_slice sl;
    if (multi_bad_nvec(who, nvec) || slice_from_device(who, sl, m, device, nr_rows, nr_cols, nr_nzeros, d_row_ptr,
                                                       d_col_ind, d_values, (hipStream_t)stream))
        return 1;
    return multi_create(m, device, op, sl, nvec);
}

static int create_host(const char *who, spmv_multi **m, int device, int op, const csr_matrix *mat, IndexType row_begin,
                       IndexType row_end, int nvec)
{
    csr_slice sl;
    if (slice_from_host(who, sl, m, mat, row_begin, row_end))
        return 1;
    *m = nullptr;
    if (multi_bad_nvec(who, nvec))
        return 1;
    return multi_create(m, device, op, sl, nvec);
}

}  // namespace spmvhw

extern "C" {

int spmv_multi_create_device(spmv_multi **m, int device, IndexType nr_rows, IndexType nr_cols, IndexType nr_nzeros,
                             const IndexType *d_row_ptr, const IndexType *d_col_ind, const ValueType *d_values,
                             int nvec, void *stream)
{
    return create_device("spmv_multi_create_device", m, device, SPMV_OP_N, nr_rows, nr_cols, nr_nzeros, d_row_ptr,
                         d_col_ind, d_values, nvec, stream);
}

int spmv_multi_create_host(spmv_multi **m, int device, const csr_matrix *mat, IndexType row_begin, IndexType row_end,
                           int nvec)
{
    return create_host("spmv_multi_create_host", m, device, SPMV_OP_N, mat, row_begin, row_end, nvec);
}

int spmv_multi_create_device_op(spmv_multi **m, int device, int op, IndexType nr_rows, IndexType nr_cols,
                                IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col_ind,
                                const ValueType *d_values, int nvec, void *stream)
{
    if (bad_op("spmv_multi_create_device_op", op))
        return 1;
    return create_device(op == SPMV_OP_N ? "spmv_multi_create_device" : "spmv_multi_create_device_op", m, device, op,
                         nr_rows, nr_cols, nr_nzeros, d_row_ptr, d_col_ind, d_values, nvec, stream);
}

int spmv_multi_create_host_op(spmv_multi **m, int device, int op, const csr_matrix *mat, IndexType row_begin,
                              IndexType row_end, int nvec)
{
    if (bad_op("spmv_multi_create_host_op", op))
        return 1;
    return create_host(op == SPMV_OP_N ? "spmv_multi_create_host" : "spmv_multi_create_host_op", m, device, op, mat,
                       row_begin, row_end, nvec);
}

int spmv_multi_run(const spmv_multi *m, const ValueType *d_X, ValueType *d_Y, void *stream)
{
    // a pointer that is not even aligned to one value is misaligned for every nvec: refused
    // before the handle is looked at
    if (uintptr_t(d_X) % sizeof(ValueType) || uintptr_t(d_Y) % sizeof(ValueType)) {
        set_error("spmv_multi_run: misaligned X or Y (not a multiple of sizeof(ValueType))");
        return 1;
    }
    if (!m) {
        set_error("spmv_multi_run: null handle");
        return 1;
    }
    // a row of X or Y is nvec values: min(16, nvec * sizeof(ValueType)) bytes for nvec 1, 2, 4, 8;
    // for the other counts (fallback only) the largest power of two that divides a row, up to 16
    const uintptr_t rowb = uintptr_t(m->nvec) * sizeof(ValueType);
    const uintptr_t align = std::min<uintptr_t>(16, rowb & (~rowb + 1));
    if (uintptr_t(d_X) % align || uintptr_t(d_Y) % align) {
        set_error("spmv_multi_run: misaligned X or Y (need " + std::to_string(align) + " bytes for this nvec)");
        return 1;
    }
    const spmv_plan &p = *m->plan;
    hipStream_t s = (hipStream_t)stream;
    if (p.nr_rows == 0)
        return 0;
    if (!d_X || !d_Y) {
        set_error("spmv_multi_run: null X or Y");
        return 1;
    }
    SPMV_TRY(hipSetDevice(p.device));
    if (m->native) {
        SPMV_TRY(p.kernel == kKernelSweep ? launch_sweep_multi(p, m->nvec, d_X, d_Y, s)
                                          : launch_slices_multi(p, m->nvec, d_X, d_Y, s));
        return 0;
    }
    if (m->nvec == 1)
        return spmv_plan_run(&p, d_X, d_Y, stream);
    const uint32_t K = (uint32_t)m->nvec;
    const uint64_t nx = uint64_t(p.nr_cols) * K, ny = uint64_t(p.nr_rows) * K;
    if (nx) {
        hipLaunchKernelGGL(k_multi_split, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, d_X, m->d_xs,
                           uint64_t(p.nr_cols), K);
        SPMV_TRY(hipGetLastError());
    }
    for (uint32_t j = 0; j < K; ++j)
        if (spmv_plan_run(&p, m->d_xs + uint64_t(j) * p.nr_cols, m->d_ys + uint64_t(j) * p.nr_rows, stream))
            return 1;
    hipLaunchKernelGGL(k_multi_join, dim3((unsigned)((ny + 255) / 256)), dim3(256), 0, s, (const ValueType *)m->d_ys,
                       d_Y, uint64_t(p.nr_rows), K);
    SPMV_TRY(hipGetLastError());
    return 0;
}

int spmv_multi_get_stats(const spmv_multi *m, spmv_multi_stats *st)
{
    if (!m || !st) {
        set_error("spmv_multi_get_stats: null argument");
        return 1;
    }
    spmv_plan_stats ps;
    if (spmv_plan_get_stats(m->plan, &ps))
        return 1;
    std::memset(st, 0, sizeof(*st));
    const uint64_t vecs = uint64_t(m->nvec) * (ps.nr_cols + ps.nr_rows) * sizeof(ValueType);
    st->nr_rows = ps.nr_rows;
    st->nr_cols = ps.nr_cols;
    st->nr_nzeros = ps.nr_nzeros;
    st->device_bytes = ps.device_bytes + (m->d_xs ? vecs : 0);
    st->algorithmic_bytes = ps.nr_nzeros * (sizeof(ValueType) + 4) + (ps.nr_rows + 1) * 4 + vecs;
    st->device = ps.device;
    st->nvec = m->nvec;
    st->native = m->native ? 1 : 0;
    st->kernel = ps.kernel;
    st->format = ps.format;
    return 0;
}

int spmv_multi_get_plan_stats(const spmv_multi *m, spmv_plan_stats *st)
{
    if (!m || !st) {
        set_error("spmv_multi_get_plan_stats: null argument");
        return 1;
    }
    return spmv_plan_get_stats(m->plan, st);
}

void spmv_multi_destroy(spmv_multi *m) { delete m; }

}  // extern "C"
