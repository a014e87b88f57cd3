// Device CSR transpose (include/csr_hw_wrapper.h, spmv_csr_transpose_device) and the transposed
// slices behind the op = SPMV_OP_T plans (plan.cpp, multi.cpp). DESIGN.md §15.
//
// Stable and deterministic, O(nnz) work plus one radix sort over the bits nr_cols - 1 needs:
//   1. k_tr_rows     entry e -> (its row, e): the row is the largest r with row_ptr[r] <= e (an
//                    upper bound minus one, so empty rows before r never claim the entry);
//                    neighbouring entries search neighbouring rows, the row_ptr lines stay cached
//   2. SortPairs     keys = the columns (read in place), values = the entry indices. The radix
//                    sort is stable: inside one column the entry indices stay ascending, which
//                    is A's CSR entry order. The sorted keys land in the output's t_col_ind as
//                    scratch (the gather overwrites them afterwards).
//   3. k_tr_row_ptr  t_row_ptr[c] = first position of the sorted keys with key >= c (c = 0 ..
//                    nr_cols): no counters, no atomics, no scan, every element written once
//   4. k_tr_gather   t_col_ind[k] = row[idx[k]], t_values[k] = values[idx[k]]
// Nothing depends on the order in which workgroups run, so the three output arrays are the same
// bits on every run. Temporaries: 12 bytes per non-zero (row ids, entry indices in and out),
// nr_rows + 1 row_ptr words and the sort's own workspace, all freed before the call returns.
// Limit: at most 2^31 - 1 non-zeros per call (hipcub item counts are int where blocked.hip sorts,
// and the 64-bit path could not be tested in a suite that runs in seconds).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>

#include "spmv_internal.hpp"

namespace spmvhw {

namespace {

constexpr int kTrThreads = 256;
constexpr uint64_t kTrMaxNnz = 0x7FFFFFFFull;

__global__ void k_tr_rows(const IndexType *__restrict__ rp, uint32_t n, uint64_t nnz, uint32_t *__restrict__ row,
                          uint32_t *__restrict__ idx)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz)
        return;
    // rp[lo] <= e < rp[hi] holds throughout (rp[0] = 0, rp[n] = nnz); lo ends as the row
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rp[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    row[e] = lo;
    idx[e] = (uint32_t)e;
}

__global__ void k_tr_row_ptr(const uint32_t *__restrict__ keys, uint64_t nnz, uint64_t ncols_plus_1,
                             IndexType *__restrict__ t_rp)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncols_plus_1)
        return;
    uint64_t lo = 0, hi = nnz;  // first k in [0, nnz] with keys[k] >= c
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    t_rp[c] = (IndexType)lo;
}

__global__ void k_tr_gather(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ row,
                            const ValueType *__restrict__ val, uint64_t nnz, IndexType *__restrict__ t_col,
                            ValueType *__restrict__ t_val)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz)
        return;
    const uint32_t e = __builtin_nontemporal_load(idx + k);  // streamed once; the gathers keep the caches
    t_col[k] = row[e];
    t_val[k] = val[e];
}

inline unsigned tr_blocks(uint64_t items) { return (unsigned)((items + kTrThreads - 1) / kTrThreads); }

}  // namespace

bool bad_op(const char *who, int op)
{
    if (op == SPMV_OP_N || op == SPMV_OP_T)
        return false;
    set_error(std::string(who) + ": op must be SPMV_OP_N (0) or SPMV_OP_T (1)");
    return true;
}

int check_transpose_size(const char *who, uint64_t nnz)
{
    if (nnz <= kTrMaxNnz)
        return 0;
    set_error(std::string(who) + ": the device transpose takes at most 2^31 - 1 non-zeros per call");
    return 1;
}

int csr_transpose_device(IndexType n, IndexType m, const IndexType *h_rp, const IndexType *d_col,
                         const ValueType *d_val, IndexType *d_t_rp, IndexType *d_t_col, ValueType *d_t_val,
                         hipStream_t s)
{
    const uint64_t nnz = n ? h_rp[n] : 0;
    if (check_transpose_size("csr transpose", nnz))
        return 1;
    if (!d_t_rp || (nnz && (!d_col || !d_val || !d_t_col || !d_t_val))) {
        set_error("csr transpose: null argument");
        return 1;
    }
    if (nnz == 0) {
        SPMV_TRY(hipMemsetAsync(d_t_rp, 0, (size_t(m) + 1) * sizeof(IndexType), s));
        SPMV_TRY(hipStreamSynchronize(s));
        return 0;
    }
    device_scratch bad, rp, row, i0, i1, work;
    SPMV_TRY(hipMalloc(&bad.p, sizeof(uint32_t)));
    SPMV_TRY(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    SPMV_TRY(launch_validate(d_col, nnz, m, (uint32_t *)bad.p, s));
    uint32_t h_bad = 0;
    SPMV_TRY(hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, s));
    SPMV_TRY(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("column index out of range (>= nr_cols)");
        return 1;
    }
    SPMV_TRY(hipMalloc(&rp.p, (size_t(n) + 1) * sizeof(IndexType)));
    SPMV_TRY(hipMalloc(&row.p, nnz * sizeof(uint32_t)));
    SPMV_TRY(hipMalloc(&i0.p, nnz * sizeof(uint32_t)));
    SPMV_TRY(hipMalloc(&i1.p, nnz * sizeof(uint32_t)));
    SPMV_TRY(hipMemcpyAsync(rp.p, h_rp, (size_t(n) + 1) * sizeof(IndexType), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tr_rows, dim3(tr_blocks(nnz)), dim3(kTrThreads), 0, s, (const IndexType *)rp.p, n, nnz,
                       (uint32_t *)row.p, (uint32_t *)i0.p);
    SPMV_TRY(hipGetLastError());
    int end_bit = 1;  // exactly the bits of nr_cols - 1 (validated: every key is below nr_cols)
    while (end_bit < 32 && (1ull << end_bit) < uint64_t(m))
        ++end_bit;
    size_t work_bytes = 0;
    uint32_t *keys_out = d_t_col;  // scratch until the gather writes the source rows there
    SPMV_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, work_bytes, d_col, keys_out, (const uint32_t *)i0.p,
                                                (uint32_t *)i1.p, (int)nnz, 0, end_bit, s));
    SPMV_TRY(hipMalloc(&work.p, std::max<size_t>(work_bytes, 1)));
    SPMV_TRY(hipcub::DeviceRadixSort::SortPairs(work.p, work_bytes, d_col, keys_out, (const uint32_t *)i0.p,
                                                (uint32_t *)i1.p, (int)nnz, 0, end_bit, s));
    hipLaunchKernelGGL(k_tr_row_ptr, dim3(tr_blocks(uint64_t(m) + 1)), dim3(kTrThreads), 0, s,
                       (const uint32_t *)keys_out, nnz, uint64_t(m) + 1, d_t_rp);
    SPMV_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tr_gather, dim3(tr_blocks(nnz)), dim3(kTrThreads), 0, s, (const uint32_t *)i1.p,
                       (const uint32_t *)row.p, d_val, nnz, d_t_col, d_t_val);
    SPMV_TRY(hipGetLastError());
    SPMV_TRY(hipStreamSynchronize(s));
    if (std::getenv("SPMV_HW_TRACE"))
        std::fprintf(stderr, "spmv_hw trace: csr transpose %llu nnz, temporaries %.1f MB (sort workspace %.1f MB)\n",
                     (unsigned long long)nnz, (nnz * 12.0 + (n + 1.0) * 4 + work_bytes) / 1e6, work_bytes / 1e6);
    return 0;
}

int transpose_slice(transposed_csr &t, const csr_slice &sl)
{
    const IndexType n = sl.n, m = sl.m;
    const uint64_t nnz = sl.nnz();
    hipStream_t s = (hipStream_t)sl.stream;
    if (check_transpose_size("csr transpose", nnz))
        return 1;
    device_scratch up_col, up_val, t_rp;
    const IndexType *d_col = nullptr;
    const ValueType *d_val = nullptr;
    if (slice_entries_on_device(sl, up_col, up_val, &d_col, &d_val))
        return 1;
    SPMV_TRY(hipMalloc(&t_rp.p, (size_t(m) + 1) * sizeof(IndexType)));
    SPMV_TRY(hipMalloc(&t.col.p, std::max<uint64_t>(nnz, 1) * sizeof(IndexType)));
    SPMV_TRY(hipMalloc(&t.val.p, std::max<uint64_t>(nnz, 1) * sizeof(ValueType)));
    if (csr_transpose_device(n, m, sl.rp.data(), d_col, d_val, (IndexType *)t_rp.p, (IndexType *)t.col.p,
                             (ValueType *)t.val.p, s))
        return 1;
    t.slice.n = m;
    t.slice.m = n;
    t.slice.rp.resize(size_t(m) + 1);
    t.slice.col = (const IndexType *)t.col.p;
    t.slice.val = (const ValueType *)t.val.p;
    t.slice.on_device = true;
    t.slice.stream = sl.stream;
    SPMV_TRY(hipMemcpyAsync(t.slice.rp.data(), t_rp.p, t.slice.rp.size() * sizeof(IndexType), hipMemcpyDeviceToHost, s));
    SPMV_TRY(hipStreamSynchronize(s));
    return 0;
}

}  // namespace spmvhw

using namespace spmvhw;

extern "C" int spmv_csr_transpose_device(int device, IndexType nr_rows, IndexType nr_cols, IndexType nr_nzeros,
                                         const IndexType *d_row_ptr, const IndexType *d_col_ind,
                                         const ValueType *d_values, IndexType *d_t_row_ptr, IndexType *d_t_col_ind,
                                         ValueType *d_t_values, void *stream)
{
    csr_slice sl;  // d_t_row_ptr stands where the creates have their out-handle: null is a null argument
    if (slice_from_device("spmv_csr_transpose_device", sl, d_t_row_ptr, device, nr_rows, nr_cols, nr_nzeros, d_row_ptr,
                          d_col_ind, d_values, (hipStream_t)stream) ||
        check_transpose_size("spmv_csr_transpose_device", nr_nzeros))
        return 1;
    return csr_transpose_device(sl.n, sl.m, sl.rp.data(), sl.col, sl.val, d_t_row_ptr, d_t_col_ind, d_t_values,
                                (hipStream_t)stream);
}
