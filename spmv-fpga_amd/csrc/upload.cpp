// Getting a CSR slice to the device: the staged upload of pageable host arrays, and the device
// side of the creates' slice front end (the host side is host.cpp).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <thread>

#include "spmv_internal.hpp"

namespace spmvhw {

// Host -> device copy of a pageable buffer through two pinned 32 MiB staging buffers (process
// lifetime): host threads fill one buffer while the DMA engine drains the other. A pageable
// hipMemcpy runs at ~1 GB/s here; this keeps the PCIe link busy instead.
int upload_staged(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    constexpr size_t kChunk = 32u << 20;
    if (bytes < (4u << 20)) {
        SPMV_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        SPMV_TRY(hipStreamSynchronize(s));
        return 0;
    }
    static std::mutex mu;
    static void *buf[2] = {nullptr, nullptr};
    static hipEvent_t done[2] = {nullptr, nullptr};
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < 2; ++i) {
        if (!buf[i])
            SPMV_TRY(hipHostMalloc(&buf[i], kChunk, hipHostMallocPortable));
        if (!done[i])
            SPMV_TRY(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
    }
    bool pending[2] = {false, false};
    const unsigned hc = std::thread::hardware_concurrency();
    const int T = (int)std::min(4u, hc ? hc : 1u);
    int i = 0;
    for (size_t off = 0; off < bytes; off += kChunk, i ^= 1) {
        const size_t n = std::min(kChunk, bytes - off);
        if (pending[i])
            SPMV_TRY(hipEventSynchronize(done[i]));  // the DMA out of this buffer has finished
        auto part = [&](int t) {
            const size_t b = n * t / T, e = n * (t + 1) / T;
            std::memcpy((char *)buf[i] + b, (const char *)src + off + b, e - b);
        };
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t)
            th.emplace_back(part, t);
        part(0);
        for (auto &t : th)
            t.join();
        SPMV_TRY(hipMemcpyAsync((char *)dst + off, buf[i], n, hipMemcpyHostToDevice, s));
        SPMV_TRY(hipEventRecord(done[i], s));
        pending[i] = true;
    }
    SPMV_TRY(hipStreamSynchronize(s));
    return 0;
}

int slice_from_device(const char *who, csr_slice &out, const void *handle, int device, IndexType n, IndexType m,
                      IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col, const ValueType *d_val,
                      hipStream_t stream)
{
    if (slice_device_args(who, handle, n, d_row_ptr))
        return 1;
    SPMV_TRY(hipSetDevice(device));
    out.n = n;
    out.m = m;
    out.rp.assign(size_t(n) + 1, 0u);
    if (n) {
        SPMV_TRY(hipMemcpyAsync(out.rp.data(), d_row_ptr, out.rp.size() * sizeof(IndexType), hipMemcpyDeviceToHost,
                                stream));
        SPMV_TRY(hipStreamSynchronize(stream));
    }
    out.col = d_col;
    out.val = d_val;
    out.on_device = true;
    out.stream = stream;
    return slice_rebase(who, out, &nr_nzeros);
}

int slice_entries_on_device(const csr_slice &sl, device_scratch &up_col, device_scratch &up_val,
                            const IndexType **d_col, const ValueType **d_val)
{
    *d_col = sl.col;
    *d_val = sl.val;
    const uint64_t nnz = sl.nnz();
    if (sl.on_device || !nnz)
        return 0;
    hipStream_t s = (hipStream_t)sl.stream;
    SPMV_TRY(hipMalloc(&up_col.p, nnz * sizeof(IndexType)));
    SPMV_TRY(hipMalloc(&up_val.p, nnz * sizeof(ValueType)));
    if (upload_staged(up_col.p, sl.col, nnz * sizeof(IndexType), s) ||
        upload_staged(up_val.p, sl.val, nnz * sizeof(ValueType), s))
        return 1;
    *d_col = (const IndexType *)up_col.p;
    *d_val = (const ValueType *)up_val.p;
    return 0;
}

}  // namespace spmvhw
