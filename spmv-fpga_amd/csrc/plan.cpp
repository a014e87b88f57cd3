// The plan object: the layout table's rows by kernel id, the kernel choice
// (automatic rules, SPMV_HW_KERNEL, the tuner), plan_create_from_slice, one SpMV by the plan's
// row, stats, variants, timing and the C entry points. The layouts themselves -- build,
// launch, sizes -- live beside their kernels (layout_ops, spmv_internal.hpp); the hipGraph
// forms are graph.cpp and the uploads upload.cpp.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "spmv_internal.hpp"

namespace spmvhw {

const layout_ops &layout_of(int kernel)
{
    static const layout_ops *const rows[kKernelCount] = {&tiles_layout(),   &gold_layout(),   &sweep_layout(), &fpga_layout(),
                                                         &blocked_layout(), &slices_layout(), &binned_layout()};
    return *rows[kernel];
}

// env SPMV_HW_TRACE=1: phase times of plan construction on stderr
struct PhaseTrace {
    const bool on = std::getenv("SPMV_HW_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void operator()(const char *phase, hipStream_t s)
    {
        if (!on)
            return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "spmv_hw trace: %-28s %9.3f ms (total %9.3f ms)\n", phase,
                     std::chrono::duration<double, std::milli>(now - last).count(),
                     std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// Which kernel a plan uses: env SPMV_HW_KERNEL = a row's name | tune | auto (default).
int requested_kernel()
{
    const char *e = std::getenv("SPMV_HW_KERNEL");
    if (!e || !*e || !std::strcmp(e, "auto"))
        return -1;
    if (!std::strcmp(e, "tune"))
        return kKernelTune;
    for (int k = 0; k < kKernelCount; ++k)
        if (!std::strcmp(e, layout_of(k).name))
            return k;
    return -1;
}

// Builds plan P's layout for `kernel` from the validated device CSR and loads its kernels. A
// build that returns 2 (the layout cannot hold this matrix) sends an automatic plan down the
// rows' decline chain: binned -> sweep -> tiles, slices -> tiles.
static int build_layout(spmv_plan &P, int kernel, bool automatic, const IndexType *h_row_ptr,
                        const IndexType *d_col, const ValueType *d_val, hipStream_t s)
{
    for (;;) {
        P.kernel = kernel;
        const layout_ops &L = layout_of(kernel);
        const int rc = L.build(P, h_row_ptr, d_col, d_val, s);
        if (rc == 2 && automatic && L.decline_to >= 0) {
            (void)hipGetLastError();
            kernel = L.decline_to;
            continue;
        }
        if (rc)
            return 1;
        break;
    }
    SPMV_TRY(hipStreamSynchronize(s));
    // load the code objects of the kernels this plan launches (no launch; best effort: a
    // failure here only means the first run loads them)
    layout_of(P.kernel).warm(P, s);
    (void)hipGetLastError();
    return 0;
}

int plan_create_from_slice(spmv_plan **out, int device, int op, const csr_slice &sl, int force_kernel, int multi_nvec)
{
    *out = nullptr;
    if (op == SPMV_OP_T) {  // the slice's transpose (transpose.hip) through the same construction, n x m -> m x n
        SPMV_TRY(hipSetDevice(device));
        transposed_csr t;
        if (transpose_slice(t, sl) ||
            plan_create_from_slice(out, device, SPMV_OP_N, t.slice, force_kernel, multi_nvec))
            return 1;
        (*out)->op = SPMV_OP_T;
        return 0;
    }
    PhaseTrace trace;
    const IndexType nr_rows = sl.n, nr_cols = sl.m;
    const IndexType *h_row_ptr = sl.rp.data();
    hipStream_t s = (hipStream_t)sl.stream;
    const uint64_t nnz = sl.nnz();
    uint64_t nzr = 0;
    for (IndexType r = 0; r < nr_rows; ++r)
        nzr += h_row_ptr[r + 1] > h_row_ptr[r];
    if (nnz > 0 && nr_cols == 0) {
        set_error("matrix has non-zeros but zero columns");
        return 1;
    }
    SPMV_TRY(hipSetDevice(device));

    plan_seed seed;
    seed.device = device;
    seed.nr_rows = nr_rows;
    seed.nr_cols = nr_cols;
    seed.nnz = nnz;
    seed.nzr = nzr;
    seed.has_empty = nzr < nr_rows;

    // device copies of the CSR entries (host path: upload), validated before any kernel gathers
    device_scratch tcol, tval, trp, tbad;
    const IndexType *d_col = nullptr;
    const ValueType *d_val = nullptr;
    if (slice_entries_on_device(sl, tcol, tval, &d_col, &d_val))
        return 1;
    trace("row_ptr scan + upload", s);
    if (nnz) {
        SPMV_TRY(hipMalloc(&tbad.p, sizeof(uint32_t)));
        SPMV_TRY(hipMemsetAsync(tbad.p, 0, sizeof(uint32_t), s));
        SPMV_TRY(launch_validate(d_col, nnz, nr_cols, (uint32_t *)tbad.p, s));
        uint32_t bad = 0;
        SPMV_TRY(hipMemcpyAsync(&bad, tbad.p, sizeof(bad), hipMemcpyDeviceToHost, s));
        SPMV_TRY(hipStreamSynchronize(s));
        if (bad) {
            set_error("column index out of range (>= nr_cols)");
            return 1;
        }
    }

    const int requested = force_kernel >= 0 ? force_kernel : requested_kernel();
    int kernel = requested;
    const bool tune = kernel == kKernelTune;
    if (kernel == -1 || tune) {  // (tune: the automatic choice is the preferred candidate)
        // automatic choice: the sweep pays once x outgrows ~half an XCD's L2 and the columns of a
        // row are scattered: fewer than 30 % of the consecutive column pairs of sampled rows lie
        // < 64 apart (random: ~0; 2-D 5-point stencil 0.5, 3-D 7-point 0.33, 27-point 0.69, where
        // the (clustered) tile layout is as fast or faster). Measured on power-law matrices with
        // 16 nnz/row (profiles/r01_ab_variants.jsonl): tie at x = 1.6 MB, sweep 1.2x faster at
        // 2.4 MB, 2.3x at 8 MB, 3.4x at 16 MB, 3.9x at 80 MB.
        kernel = kKernelTiles;
        if (nnz && uint64_t(nr_cols) * sizeof(ValueType) >= (2ull << 20) && nnz >= 16ull * kSweepThreads) {
            SPMV_TRY(hipMalloc(&trp.p, (size_t(nr_rows) + 1) * sizeof(IndexType)));
            SPMV_TRY(hipMemcpyAsync(trp.p, h_row_ptr, (size_t(nr_rows) + 1) * sizeof(IndexType),
                                    hipMemcpyHostToDevice, s));
            if (probe_locality((const IndexType *)trp.p, d_col, nr_rows, s, &seed.locality))
                return 1;
            if (seed.locality < 0.3)
                kernel = kKernelSweep;
        }
        // fp32, scattered, x of >= 20 MB: the two-pass binned kernel (binned.hip) streams 15-16 B
        // per non-zero instead of gathering x lines (skewed matrices excepted, build_binned). Measured on the power-law generator
        // (profiles/r02_binned.jsonl, profiles/r02_strong_binned.jsonl): square n x n, 16n nnz:
        // 4M 0.203 vs 0.199 ms (sweep), 6M 0.317 vs 0.374, 10M 0.457 vs 0.616, 20M 0.964 vs
        // 1.450; row slices of the 10M x 10M matrix (x stays 40 MB): 5M rows / 80M nnz 0.251
        // vs 0.312, 2.5M / 40M 0.144 vs 0.178, 1.25M / 20M 0.093 vs 0.106. In fp64 (27-28 B per
        // non-zero) the sweep stays as fast or faster (10M: binned 0.80-0.86 vs 0.78-0.80 ms;
        // slices slower).
        // Its pass 2 adds in timing order; SPMV_SWEEP_DETERMINISTIC=1 asks for fixed bits, which
        // the turn-ordered sweep gives, so the switch keeps the sweep.
        const char *det = std::getenv("SPMV_SWEEP_DETERMINISTIC");
        if (kernel == kKernelSweep && sizeof(ValueType) == 4 && nr_cols >= 5000000u && nnz >= 16000000ull &&
            !(det && det[0] == '1'))
            kernel = kKernelBinned;
    }
    const int auto_kernel = kernel;
    if (tune)
        kernel = kKernelTune;
    trace("validate + kernel choice", s);
    if (const char *t = ablation_env("SPMV_SWEEP_THREADS")) {
        const int v = std::atoi(t);
        if (v == 256 || v == 512 || v == 1024)
            seed.sweep_threads = v;
    }
    // every layout attempt starts from the seed alone
    auto fresh = [&]() { return std::unique_ptr<spmv_plan>(new spmv_plan(seed)); };
    std::unique_ptr<spmv_plan> p = fresh();
    if (kernel == kKernelTune) {
        // build the tile, sweep, slice and binned layouts (the rows with a tune_slot) one at a time
        // and time each on this matrix (time_layout: median of graph-replayed samples). The
        // candidates go in preference order -- the automatic choice first, then by slot: tiles,
        // sweep, slices, binned -- and a later one
        // replaces the kept layout only when it is more than 3 % faster, so two layouts within
        // the timer's noise of each other cannot trade places between two builds of one matrix.
        // Only the kept layout and the candidate are resident; a candidate whose build fails
        // (e.g. out of memory) is dropped, not a plan error. With SPMV_SWEEP_DETERMINISTIC=1 the
        // binned layout (pass-2 adds in timing order) is not a candidate: the switch promises
        // fixed bits.
        const char *det = std::getenv("SPMV_SWEEP_DETERMINISTIC");
        const bool fixed_bits = det && det[0] == '1';
        constexpr double kTuneBand = 0.97;
        device_scratch tx, ty;
        SPMV_TRY(hipMalloc(&tx.p, std::max<size_t>(nr_cols, 1) * sizeof(ValueType)));
        SPMV_TRY(hipMalloc(&ty.p, std::max<size_t>(nr_rows, 1) * sizeof(ValueType)));
        SPMV_TRY(hipMemsetAsync(tx.p, 0, std::max<size_t>(nr_cols, 1) * sizeof(ValueType), s));
        std::vector<int> order = {auto_kernel};
        for (int k = 0; k < kKernelCount; ++k)  // (the slots ascend with the kernel ids)
            if (layout_of(k).tune_slot >= 0 && k != auto_kernel)
                order.push_back(k);
        double tuned[4] = {1e30, 1e30, 1e30, 1e30};
        std::unique_ptr<spmv_plan> kept;
        double kept_ms = 1e30;
        for (int k : order) {
            if (k == kKernelBinned && fixed_bits)  // (this and the padding limit below: policy, like the automatic rules)
                continue;
            std::unique_ptr<spmv_plan> q = fresh();
            if (k == kKernelSlices)
                q->slices.pad_limit = 2.0;  // a slice layout padded beyond 2x is built as tiles instead
            double t = 1e30;
            if (build_layout(*q, k, true, h_row_ptr, d_col, d_val, s) ||
                time_layout(*q, (const ValueType *)tx.p, (ValueType *)ty.p, s, &t)) {
                q.reset();  // not a candidate
                (void)hipGetLastError();
                continue;
            }
            tuned[layout_of(k).tune_slot] = t;
            if (!kept || t < kTuneBand * kept_ms) {
                kept.swap(q);
                kept_ms = t;
            }
        }
        if (!kept) {  // every candidate failed: the tiles, untimed (their error is the plan's)
            if (build_layout(*p, kKernelTiles, true, h_row_ptr, d_col, d_val, s))
                return 1;
        } else {
            p.swap(kept);
        }
        if (std::getenv("SPMV_HW_TRACE"))
            std::fprintf(stderr, "spmv_hw trace: tune ms tiles %.4f sweep %.4f slices %.4f binned %.4f -> kernel %d\n",
                         tuned[0], tuned[1], tuned[2], tuned[3], p->kernel);
        for (int c = 0; c < 4; ++c)
            p->tuned_ms[c] = tuned[c];
        trace("tune: build + time each", s);
    } else if (requested < 0 && kernel == kKernelTiles && nnz >= 65536) {
        // automatic, local columns: the slice layout when rows of a 64-row slice have about the
        // same length (<= 15 % padding) and every slot fits 16-bit (or clustered 16-bit) offsets
        // -- finite-element / stencil-like matrices, where it is 7-14 % faster than the tiles
        // (fp32: 24-34 %, profiles/r01_ab_variants.jsonl); in fp64, 8-bit spans (narrow bands)
        // keep the tiles, which gather a band's x from fewer lines per instruction (the fp32
        // band is 13 % faster in slices)
        std::unique_ptr<spmv_plan> r = fresh();
        r->slices.pad_limit = 1.15;
        const int rc = build_layout(*r, kKernelSlices, true, h_row_ptr, d_col, d_val, s);
        if (rc == 0 && r->kernel == kKernelSlices &&
            (r->slices.off_bytes == 2 || (r->slices.off_bytes == 1 && sizeof(ValueType) == 4)) &&
            double(r->slices.slots) * kWave <= 1.15 * double(nnz)) {
            p.swap(r);
        } else if (rc == 0 && r->kernel == kKernelTiles) {  // padding too high: built as tiles
            r->slices.pad_limit = 0.0;
            p.swap(r);
        } else {
            r.reset();
            (void)hipGetLastError();
            if (build_layout(*p, kKernelTiles, true, h_row_ptr, d_col, d_val, s))
                return 1;
        }
        trace(layout_of(p->kernel).trace_label, s);
    } else {
        // spmv_multi's one-pass sweep (multi_nvec > 1), on a matrix that takes the sweep or the
        // binned kernel: tried first when the unsplit panels of multi_nvec accumulators per row
        // fill a round of resident workgroups; a build that declines or fails leaves the ordinary
        // plan below
        if (multi_nvec > 1 && requested < 0 && (kernel == kKernelSweep || kernel == kKernelBinned)) {
            const uint64_t wgs = (uint64_t)device_cu_count(device) * (1024 / p->sweep_threads);
            if (min_panels(nr_rows, sweep_rmax(p->sweep_threads, 8, multi_nvec)) >= wgs) {
                std::unique_ptr<spmv_plan> r = fresh();
                r->sweep.nvec = multi_nvec;
                if (build_layout(*r, kKernelSweep, false, h_row_ptr, d_col, d_val, s) == 0) {
                    trace("build multi-vector sweep layout", s);
                    *out = r.release();
                    return 0;
                }
                r.reset();
                (void)hipGetLastError();
                // (the sort was paid for nothing: say so where build times are read)
                if (trace.on)
                    std::fprintf(stderr, "spmv_hw trace: multi-vector sweep layout declined: %s\n", get_error());
                trace("multi-vector sweep layout (declined)", s);
            }
        }
        if (kernel == kKernelBinned && requested < 0) {
            p->binned.skew_limit = 2.0;  // automatic: skewed matrices stay on the sweep
            // and so do matrices with a row above 0.3x a panel's mean entries: 2M x 6M fp32 with
            // 64 rows of L (profiles/r03e_skew_rowlimit.jsonl; L / mean 0.12, 0.24, 0.44, 0.81):
            // binned 0.136 / 0.178 / 0.254 / 0.282 ms, sweep 0.155 / 0.183 / 0.225 / 0.298
            p->binned.row_limit = 0.3;
            if (const char *e = std::getenv("SPMV_BIN_ROW_LIMIT"))
                p->binned.row_limit = std::atof(e);
        }
        if (build_layout(*p, kernel, requested < 0, h_row_ptr, d_col, d_val, s))
            return 1;
        trace(layout_of(p->kernel).trace_label, s);
    }
    *out = p.release();
    return 0;
}

int timing_begin(spmv_plan *p, hipStream_t s, hipEvent_t *e1)
{
    while (p->timing.used + 2 > p->timing.ev.size()) {
        hipEvent_t e;
        SPMV_TRY(hipEventCreate(&e));
        p->timing.ev.push_back(e);
    }
    const hipEvent_t e0 = p->timing.ev[p->timing.used];
    *e1 = p->timing.ev[p->timing.used + 1];
    p->timing.used += 2;
    SPMV_TRY(hipEventRecord(e0, s));
    return 0;
}

int run_impl(spmv_plan *p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool timing)
{
    if (p->nr_rows == 0)
        return 0;
    const layout_ops &L = layout_of(p->kernel);
    if (L.before)
        SPMV_TRY(L.before(*p, d_y, s));
    hipEvent_t e1 = nullptr;
    if (timing && timing_begin(p, s, &e1))
        return 1;
    SPMV_TRY(L.launch(*p, d_x, d_y, s));
    if (timing)
        SPMV_TRY(hipEventRecord(e1, s));
    if (L.after)
        SPMV_TRY(L.after(*p, d_y, s));
    return 0;
}

}  // namespace spmvhw

using namespace spmvhw;

uint64_t spmv_plan::device_bytes() const { return layout_of(kernel).device_bytes(*this); }

// z*(sizeof(val)+4) + (n+1)*4 + m*sizeof(val) + n*sizeof(val)
uint64_t spmv_plan::algorithmic_bytes() const
{
    return nnz * (sizeof(ValueType) + 4) + (uint64_t(nr_rows) + 1) * 4 +
           uint64_t(nr_cols) * sizeof(ValueType) + uint64_t(nr_rows) * sizeof(ValueType);
}

// The four plan creates: `who` names the caller in the messages (op = SPMV_OP_N through an _op
// function is the function without an op, and reports as it)
static int create_device(const char *who, spmv_plan **plan, int device, int op, IndexType nr_rows, IndexType nr_cols,
                         IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col_ind,
                         const ValueType *d_values, void *stream)
{
    csr_slice sl;
    if (slice_from_device(who, sl, plan, device, nr_rows, nr_cols, nr_nzeros, d_row_ptr, d_col_ind, d_values,
                          (hipStream_t)stream))
        return 1;
    return plan_create_from_slice(plan, device, op, sl);
}

static int create_host(const char *who, spmv_plan **plan, int device, int op, const csr_matrix *m, IndexType row_begin,
                       IndexType row_end)
{
    csr_slice sl;
    if (slice_from_host(who, sl, plan, m, row_begin, row_end))
        return 1;
    return plan_create_from_slice(plan, device, op, sl);
}

extern "C" {

int spmv_plan_create_device(spmv_plan **plan, int device, IndexType nr_rows, IndexType nr_cols,
                            IndexType nr_nzeros, const IndexType *d_row_ptr,
                            const IndexType *d_col_ind, const ValueType *d_values, void *stream)
{
    return create_device("spmv_plan_create_device", plan, device, SPMV_OP_N, nr_rows, nr_cols, nr_nzeros, d_row_ptr,
                         d_col_ind, d_values, stream);
}

int spmv_plan_create_host(spmv_plan **plan, int device, const csr_matrix *m, IndexType row_begin,
                          IndexType row_end)
{
    return create_host("spmv_plan_create_host", plan, device, SPMV_OP_N, m, row_begin, row_end);
}

int spmv_plan_create_device_op(spmv_plan **plan, int device, int op, IndexType nr_rows, IndexType nr_cols,
                               IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col_ind,
                               const ValueType *d_values, void *stream)
{
    if (bad_op("spmv_plan_create_device_op", op))
        return 1;
    return create_device(op == SPMV_OP_N ? "spmv_plan_create_device" : "spmv_plan_create_device_op", plan, device, op,
                         nr_rows, nr_cols, nr_nzeros, d_row_ptr, d_col_ind, d_values, stream);
}

int spmv_plan_create_host_op(spmv_plan **plan, int device, int op, const csr_matrix *m, IndexType row_begin,
                             IndexType row_end)
{
    if (bad_op("spmv_plan_create_host_op", op))
        return 1;
    return create_host(op == SPMV_OP_N ? "spmv_plan_create_host" : "spmv_plan_create_host_op", plan, device, op, m,
                       row_begin, row_end);
}

int spmv_plan_get_op(const spmv_plan *plan, int *op)
{
    if (!plan || !op) {
        set_error("spmv_plan_get_op: null argument");
        return 1;
    }
    *op = plan->op;
    return 0;
}

int spmv_plan_run(const spmv_plan *cp, const ValueType *d_x, ValueType *d_y, void *stream)
{
    if (!cp) {
        set_error("spmv_plan_run: null plan");
        return 1;
    }
    spmv_plan *p = const_cast<spmv_plan *>(cp);
    SPMV_TRY(hipSetDevice(p->device));
    return run_impl(p, d_x, d_y, (hipStream_t)stream, p->timing.on);
}

int spmv_plan_get_stats(const spmv_plan *p, spmv_plan_stats *st)
{
    if (!p || !st) {
        set_error("spmv_plan_get_stats: null argument");
        return 1;
    }
    const layout_ops &L = layout_of(p->kernel);
    std::memset(st, 0, sizeof(*st));
    st->nr_rows = p->nr_rows;
    st->nr_cols = p->nr_cols;
    st->nr_nzeros = p->nnz;
    st->nr_nonempty_rows = p->nzr;
    // work units of the main kernel: tiles, sweep units (panel pieces), or long rows (gold)
    st->nr_tiles = L.units(*p);
    st->tile_nnz = L.unit_nnz(*p);
    st->device_bytes = p->device_bytes();
    st->algorithmic_bytes = p->algorithmic_bytes();
    st->device = p->device;
    st->kernel = p->kernel;
    st->blocks = L.blocks(*p);
    // the layout's bits, and how spmv_plan_run_graph would capture the plan (256 behind, 512 DAG)
    const int form = graph_form(p);
    st->format = L.format_bits(*p) | (form == 2 ? 256 : form == 1 ? 512 : 0);
    return 0;
}

int spmv_plan_set_variant(spmv_plan *p, int variant)
{
    if (!p || variant < 0 || (variant > 63 && variant != kSweepTurn && variant != kSweepTurnOrdered)) {
        set_error("spmv_plan_set_variant: bad arguments");
        return 1;
    }
    const layout_ops &L = layout_of(p->kernel);
#ifndef SPMV_ABLATIONS
    // The product library takes only what a caller needs (the reference exposes no tuning
    // surface, csr_hw_wrapper.h:9-17): 0 = the plan's default kernel form (the sweep's default is
    // 28, also accepted by number), the sweep's deterministic kernel 94 (bitwise reproducible y,
    // the form of SPMV_SWEEP_DETERMINISTIC=1), and binned 1 / 2 (segment offsets rebased past
    // 2^31 / 2^32: the same y, for the tests of the 64-bit offset path) -- the rows'
    // product_variants. Every other variant is a
    // performance experiment or an ablation (some give a wrong y by design) and exists only in
    // the tools library built with -DSPMV_ABLATIONS (Makefile target `ablations`).
    if (variant != 0 && variant != L.product_variants[0] && variant != L.product_variants[1]) {
        set_error("spmv_plan_set_variant: measurement variant (tools library only)");
        return 1;
    }
#endif
    if (L.set_variant(*p, variant))
        return 1;
    // a graph captured with the previous variant must not be replayed
    if (p->graph.exec) {
        (void)hipSetDevice(p->device);
        (void)p->graph.drop_exec();
    }
    return 0;
}

int spmv_plan_set_timing(spmv_plan *p, int enable)
{
    if (!p) {
        set_error("spmv_plan_set_timing: null plan");
        return 1;
    }
    p->timing.on = enable != 0;
    p->timing.used = 0;
    return 0;
}

int spmv_plan_get_timing(spmv_plan *p, double *mean_ms, double *total_ms, int *launches)
{
    if (!p) {
        set_error("spmv_plan_get_timing: null plan");
        return 1;
    }
    SPMV_TRY(hipSetDevice(p->device));
    double tot = 0.0;
    int n = 0;
    for (size_t i = 0; i + 1 < p->timing.used; i += 2) {
        SPMV_TRY(hipEventSynchronize(p->timing.ev[i + 1]));
        float ms = 0.f;
        SPMV_TRY(hipEventElapsedTime(&ms, p->timing.ev[i], p->timing.ev[i + 1]));
        tot += ms;
        ++n;
    }
    p->timing.used = 0;
    if (mean_ms)
        *mean_ms = n ? tot / n : 0.0;
    if (total_ms)
        *total_ms = tot;
    if (launches)
        *launches = n;
    return 0;
}

void spmv_plan_destroy(spmv_plan *p) { delete p; }

}  // extern "C"
