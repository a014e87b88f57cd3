// spmv_multi's second native form: the panel sweep (sweep.hip) with K accumulators per row.
//
// Y = A X for K = 2, 4 or 8 right-hand sides in one pass over a scattered matrix, X and Y
// row-major (X[c * K + j]). The layout is the sweep build's unpacked one, sized for K
// accumulators per row (build_sweep with spmv_plan::sweep.nvec = K, never split): s_col u32,
// s_row u16, s_val V per entry, panels contiguous and padded to whole 128-entry chunks, ascending
// column per panel; panel_row u32[P + 1]; unit_ent u32[P + 1] (one unit per panel, so it holds
// every panel's first padded entry). One workgroup owns one panel: its R x K sums live in LDS as
// doubles (vector-major, ylds[j * (R + 1) + row]), every entry gathers the K consecutive values of its
// column's row of X in 16-byte loads and makes K LDS adds, and the panel's R * K sums leave as
// one contiguous run of Y. The adds land in timing order: Y is not bitwise reproducible from run
// to run, as the single-vector sweep's y is not.
#include "spmv_internal.hpp"

namespace spmvhw {

typedef double mf64x2 __attribute__((ext_vector_type(2)));
typedef float mf32x2 __attribute__((ext_vector_type(2)));
typedef float mf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mu32x2 __attribute__((ext_vector_type(2)));
typedef uint16_t mu16x2 __attribute__((ext_vector_type(2)));

// the K values of row c of X (16-byte aligned rows: spmv_multi_run checks X)
template <int K>
__device__ __forceinline__ void gather_row(const double *__restrict__ X, uint32_t c, double (&o)[K])
{
    const mf64x2 *src = reinterpret_cast<const mf64x2 *>(X + (uint64_t)c * K);
#pragma unroll
    for (int j = 0; j < K / 2; ++j) {
        const mf64x2 a = src[j];
        o[2 * j] = a.x;
        o[2 * j + 1] = a.y;
    }
}
template <int K>
__device__ __forceinline__ void gather_row(const float *__restrict__ X, uint32_t c, float (&o)[K])
{
    if constexpr (K == 2) {
        const mf32x2 a = *reinterpret_cast<const mf32x2 *>(X + (uint64_t)c * 2);
        o[0] = a.x;
        o[1] = a.y;
    } else {
        const mf32x4 *src = reinterpret_cast<const mf32x4 *>(X + (uint64_t)c * K);
#pragma unroll
        for (int j = 0; j < K / 4; ++j) {
            const mf32x4 a = src[j];
            o[4 * j] = a.x;
            o[4 * j + 1] = a.y;
            o[4 * j + 2] = a.z;
            o[4 * j + 3] = a.w;
        }
    }
}

// Two entries per thread per group (entry ranges are whole 128-entry chunks, so a pair is never
// cut), Q groups per workgroup iteration, a barrier after every iteration so that the waves stay
// on one column window (without it the single-vector sweep measured 1.26 against 0.65 ms, §4).
// Branch-free tail as in k_spmv_sweep: a group past the panel's end re-reads the panel's last pair
// and adds into the scratch row R, which is never stored.
// VM: the accumulators vector-major, ylds[j * (R + 1) + row] (default), instead of row-major
// ylds[row * K + j]. Row-major, the 64 lanes of add j address byte (row * K + j) * 8: modulo 256
// only 32 / K of the 32 eight-byte positions, where vector-major reaches all 32 like the
// single-vector sweep. Vector-major measured 1.1-1.8x faster at K = 8 and up to 1.15x at K = 4
// (equal at K = 2; that bank conflicts are the cause is a supposition from this
// arithmetic, no LDS counters were collected). The write-out reads LDS with stride R + 1 and
// still stores Y contiguously.
template <typename V, int K, int T, int Q, bool VM>
__global__ __launch_bounds__(T) void k_spmv_sweep_multi(
    const uint32_t *__restrict__ col, const uint16_t *__restrict__ row, const V *__restrict__ val,
    const uint32_t *__restrict__ panel_row, const uint32_t *__restrict__ panel_ent, const V *__restrict__ X,
    V *__restrict__ Y)
{
    constexpr int E = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *ylds = reinterpret_cast<double *>(smem);
    const uint32_t p = blockIdx.x;
    const uint32_t r0 = panel_row[p], R = panel_row[p + 1] - r0;
    const uint64_t e0 = panel_ent[p], e1 = panel_ent[p + 1];
    const uint32_t nacc = (R + 1) * K;  // (R_max + 1) * K <= 20448: 32 bits hold it
    for (uint32_t i = threadIdx.x; i < nacc; i += T)
        ylds[i] = 0.0;
    __syncthreads();
    constexpr uint64_t kGroup = (uint64_t)E * T;
    const uint64_t elast = e1 > e0 ? e1 - E : e0;
    for (uint64_t base = e0; base < e1; base += Q * kGroup) {
        mu32x2 c[Q];
        mu16x2 r[Q];
        V v[Q][E];
        bool ok[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            uint64_t e = base + q * kGroup + (uint64_t)E * threadIdx.x;
            ok[q] = e < e1;
            e = ok[q] ? e : elast;
            c[q] = __builtin_nontemporal_load(reinterpret_cast<const mu32x2 *>(col + e));
            r[q] = __builtin_nontemporal_load(reinterpret_cast<const mu16x2 *>(row + e));
            if constexpr (sizeof(V) == 8) {
                const mf64x2 a = __builtin_nontemporal_load(reinterpret_cast<const mf64x2 *>(val + e));
                v[q][0] = a.x;
                v[q][1] = a.y;
            } else {
                const mf32x2 a = __builtin_nontemporal_load(reinterpret_cast<const mf32x2 *>(val + e));
                v[q][0] = a.x;
                v[q][1] = a.y;
            }
        }
        V xv[Q][E][K];
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int i = 0; i < E; ++i)
                gather_row<K>(X, c[q][i], xv[q][i]);
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const uint32_t rr = ok[q] ? (uint32_t)r[q][i] : R;
#pragma unroll
                for (int j = 0; j < K; ++j)
                    atomicAdd(ylds + (VM ? j * (R + 1) + rr : rr * K + j), double(v[q][i]) * double(xv[q][i][j]));
            }
        __syncthreads();
    }
    __syncthreads();
    V *dst = Y + (uint64_t)r0 * K;
    for (uint32_t i = threadIdx.x; i < R * K; i += T)
        dst[i] = V(ylds[VM ? (i % K) * (R + 1) + i / K : i]);
}

// The compile-time handles of the measurements in DESIGN.md §14: gather loads in flight per lane
// and the accumulator layout
#ifndef SPMV_MULTI_SWEEP_DEPTH
#define SPMV_MULTI_SWEEP_DEPTH 8
#endif
#ifndef SPMV_MULTI_SWEEP_VMAJOR
#define SPMV_MULTI_SWEEP_VMAJOR 1
#endif
// Groups per iteration: 2 entries * Q * (16-byte loads per row of X) = SPMV_MULTI_SWEEP_DEPTH
// gathers in flight per lane (8: the depth the slice kernel's multi-vector form settled on)
template <typename V, int K>
constexpr int sweep_multi_groups()
{
    constexpr int loads = K * (int)sizeof(V) / 16 ? K * (int)sizeof(V) / 16 : 1;
    return SPMV_MULTI_SWEEP_DEPTH / 2 / loads ? SPMV_MULTI_SWEEP_DEPTH / 2 / loads : 1;
}

template <int K, int T>
static void launch_sweep_multi_t(const spmv_plan &p, const ValueType *d_X, ValueType *d_Y, hipStream_t s, bool warm)
{
    const sweep_state &w = p.sweep;
    const size_t lds = (size_t(p.panels.rmax) + 1) * K * sizeof(double);
    launch_or_warm(warm, k_spmv_sweep_multi<ValueType, K, T, sweep_multi_groups<ValueType, K>(), SPMV_MULTI_SWEEP_VMAJOR != 0>,
                   dim3((unsigned)p.panels.npanels), dim3(T), lds, s, (const uint32_t *)w.col.get(), (const uint16_t *)w.row.get(),
                   (const ValueType *)w.val.get(), (const uint32_t *)p.panels.row.get(), (const uint32_t *)w.unit_ent.get(), d_X,
                   d_Y);
}

template <int K>
static void launch_sweep_multi_k(const spmv_plan &p, const ValueType *d_X, ValueType *d_Y, hipStream_t s, bool warm)
{
    switch (p.sweep_threads) {
    case 256: launch_sweep_multi_t<K, 256>(p, d_X, d_Y, s, warm); break;
    case 512: launch_sweep_multi_t<K, 512>(p, d_X, d_Y, s, warm); break;
    default: launch_sweep_multi_t<K, 1024>(p, d_X, d_Y, s, warm); break;
    }
}

// d_Y[nr_rows x nvec] = A * d_X[nr_cols x nvec], both row-major, on a sweep plan built with
// sweep.nvec = nvec (2, 4 or 8): unpacked entries, one unit per panel, no partial sums
hipError_t launch_sweep_multi(const spmv_plan &p, int nvec, const ValueType *d_X, ValueType *d_Y, hipStream_t s,
                              bool warm)
{
    if (p.kernel != kKernelSweep || p.sweep.nvec != nvec || (nvec != 2 && nvec != 4 && nvec != 8) || p.sweep.packed ||
        p.sweep.split != 1 || p.sweep.nunits != p.panels.npanels || p.sweep.acc_bytes != 8)
        return hipErrorInvalidValue;
    if (p.panels.npanels == 0)
        return hipSuccess;
    if (nvec == 2)
        launch_sweep_multi_k<2>(p, d_X, d_Y, s, warm);
    else if (nvec == 4)
        launch_sweep_multi_k<4>(p, d_X, d_Y, s, warm);
    else
        launch_sweep_multi_k<8>(p, d_X, d_Y, s, warm);
    return hipGetLastError();
}

}  // namespace spmvhw
