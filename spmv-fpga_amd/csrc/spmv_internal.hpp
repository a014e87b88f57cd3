// Internal declarations of libspmv_hw (not part of the C-ABI).
//
// The MI355X hw representation of one unit's row slice ("plan"), DESIGN.md §3:
//   col      u32[nnz_pad]   column index of every stored non-zero, CSR order
//   val      V[nnz_pad]     values; fp64 is pair-interleaved inside each 256-entry wave step so
//                           that every lane's 4 consecutive entries arrive by two fully coalesced
//                           1-KiB dwordx4 wave loads (fp32 keeps CSR order: one dwordx4)
//   rowend   u32[nnz_pad/32] bit k set <=> entry k is the last entry of its row. This is the
//                           reference's "last element of row" flag (csr_hw.cpp:288-292, bit 15 of
//                           each 16-bit column field) moved to a bitmap: 1 bit/nnz instead of 16.
//   tile_info u32[ntiles+1]  (compact row index of the tile's first entry << 1) | (1 if that
//                           entry continues a row begun in an earlier tile)
//   row_id   u32[nzr]       slice row of each non-empty row; absent when no row is empty. This
//                           replaces the reference's empty_rows_bitmap scatter
//                           (csr_hw.cpp:1531-1565) with an index map.
// Entries past nnz (padding to a whole tile) have col 0, value 0 and no row-end bit.
// Narrow form (default when every tile's columns span < 65536, e.g. banded matrices): col is
// replaced by colnar u16[nnz_pad] (u8 when every span < 256) = col - tile_cbase[tile] and
// tile_cbase u32[ntiles], i.e. the reference's block-relative 16-bit column field
// (csr_hw.cpp:288-292) with a per-tile block base: 10 (9) B/nnz fp64 and 6 (5) B/nnz fp32 are
// streamed instead of 12 and 8.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "csr_hw_wrapper.h"
#include "spmv_host.hpp"

namespace spmvhw {

// (kWave, kStep, kTileSteps, kTileNnz: spmv_host.hpp, with the tile planner)
constexpr int kBlockThreads = 256;                 // 4 waves = 4 tiles per workgroup
constexpr int kSweepThreads = 1024;                // default panel-sweep workgroup (16 waves, 1/CU)
constexpr int kSweepTurn = 91;         // sweep variant: ordered LDS adds (deterministic y), the
constexpr int kSweepTurnOrdered = 94;  // form of SPMV_SWEEP_DETERMINISTIC=1; 94: adds awaited

// plan kernels (spmv_plan_stats.kernel)
constexpr int kKernelTiles = 0;  // flagged-tile wave kernel, x gathered through the caches
constexpr int kKernelGold = 1;   // spmv_gold's exact order (bitwise reference results)
constexpr int kKernelSweep = 2;  // panel sweep: y in LDS, columns swept in order (x from L2)
constexpr int kKernelFpga = 3;   // the reference FPGA path's order for (VF, block width), bitwise
constexpr int kKernelBlocked = 4;  // the same order by the reference's dataflow: x blocks in LDS,
                                   // per-block partials, block-ordered merge (blocked.hip)
constexpr int kKernelSlices = 5;   // wave per 64 rows, entries slot-major (slices.hip)
constexpr int kKernelBinned = 6;   // two passes: products per column window, summed per row panel
                                   // (propagation blocking, binned.hip)
constexpr int kGoldLong = 128;   // gold plan stats: rows longer than this count as long

// 64-lane inclusive prefix sum (the GCN DPP sequence: row_shr 1/2/3 of the source, row_shr 4/8
// with bank masks, row_bcast 15/31 with row masks); tools/delta_probe.hip checks it. Used by the
// binned kernel's row deltas and the sweep's column deltas.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v0)
{
    uint32_t v = v0;
    v += __builtin_amdgcn_update_dpp(0u, v0, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v0, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v0, 0x113, 0xf, 0xf, true);  // row_shr:3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xe, true);   // row_shr:4, banks 1-3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xc, true);   // row_shr:8, banks 2-3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);  // row_bcast:15, rows 1, 3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);  // row_bcast:31, rows 2, 3
    return v;
}

// Device memory with one owner, freed when the owner goes: a build step's scratch on scope exit,
// a plan's buffers with the plan. Not copyable, so a buffer handed to a kernel launch by mistake
// does not compile: a kernel argument is get() (or p), never the buffer.
struct device_scratch {
    void *p = nullptr;
    device_scratch() = default;
    device_scratch(const device_scratch &) = delete;
    device_scratch &operator=(const device_scratch &) = delete;
    // `bytes` of device memory; what the buffer held before is freed first
    hipError_t alloc_bytes(uint64_t bytes)
    {
        const hipError_t e = release();
        return e != hipSuccess ? e : hipMalloc(&p, bytes);
    }
    // frees early (where that bounds a build's peak memory, or before a rebuild). swap() trades the
    // memory with another buffer: a build hands the plan a finished array, and its scratch frees
    // what the plan held
    hipError_t release()
    {
        void *q = p;
        p = nullptr;
        return q ? hipFree(q) : hipSuccess;
    }
    void swap(device_scratch &other) { std::swap(p, other.p); }
    ~device_scratch() { (void)release(); }
};
// ... of `count` elements of T
template <typename T>
struct device_buf : device_scratch {
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
    hipError_t alloc(uint64_t count) { return alloc_bytes(count * sizeof(T)); }
    void swap(device_buf &other) { device_scratch::swap(other); }  // (only with its own type)
};

// ---- a plan's state, one struct per layout (DESIGN.md §3 "The layout table") ----
// A layout's file reads `panels`, `release` and its own struct; every device buffer a plan owns is
// a device_buf / device_scratch member, and a raw pointer member is borrowed (its comment says
// from whom).

// flagged tiles (kernel 0; tiles.cpp, kernels.hip): the representation in this file's head comment
struct tiles_state {
    uint64_t nnz_pad = 0, ntiles = 0;
    device_buf<uint32_t> col;
    device_scratch colnar;           // narrow form: u16 or u8 offsets from cbase (col freed)
    device_buf<uint32_t> cbase;
    int col_bytes = 4;               // 4 (col), 2 or 1 (colnar)
    bool clustered = false;          // 2-byte columns as (cluster << 14) | offset, 4 bases per tile
    bool xcd = false;                // XCD-contiguous tile order (env SPMV_TILE_XCD=1); measured
                                     // slower on stencils (+6 %), 2 % faster on banded
    device_buf<ValueType> val;
    device_buf<uint32_t> rowend, tile_info, row_id;
    device_buf<ValueType> head, tail;
    device_buf<uint32_t> cross;      // rows crossing tile boundaries: (row, first tile, last tile)
    uint64_t ncross = 0;
};

// gold order and the reference FPGA path's order (kernels 1 and 3, gold.hip): plain CSR
struct csr_state {
    device_buf<uint32_t> rp;          // rebased row_ptr[nr_rows + 1]
    device_buf<uint32_t> col;
    device_buf<ValueType> val;
    uint64_t nlong = 0;               // rows with more than kGoldLong entries (stats)
    int fpga_vf = 1;                  // kernel 3: vectorisation factor (env SPMV_FPGA_VF)
    uint32_t fpga_width = 32768;      // kernel 3: column-block width (env SPMV_FPGA_BLOCK)
                                      // (kernel 4 takes the same two: fpga_params)
};

// blocked (kernel 4, blocked.hip): entries by (block, row)
struct blocked_state {
    device_buf<ValueType> val;
    device_buf<uint16_t> col;         // block-relative columns
    uint64_t nunits = 0;              // workgroups of the main kernel
    device_buf<uint32_t> unit_block;  // block of each unit
    device_buf<uint32_t> unit_ent;    // its compact-row range
    device_buf<uint32_t> kptr;        // first entry of each compact row [nkpairs + 1]
    device_buf<uint32_t> kpos;        // partial slot of each compact row
    device_buf<uint32_t> rp2;         // row-major offsets of each row's partials [nr_rows + 1]
    device_buf<uint16_t> rl;          // row-major: chunk-local slot of each partial
    device_buf<uint32_t> chunk_row;   // row ranges of the merge chunks [nchunks + 1]
    device_buf<ValueType> part;       // block partials (scratch)
    uint64_t nkpairs = 0, nchunks = 0;
    bool xlds = false;                // x block staged in LDS (W * sizeof(V) <= 128 KiB)
};

// slices (kernel 5, slices.hip): slot-major entries
struct slices_state {
    device_buf<ValueType> val;
    device_scratch off;               // per entry: off_bytes-wide column offsets
    device_buf<uint32_t> slot_off;    // slots of each 64-row slice [nslices + 1]
    device_buf<uint32_t> sbase;       // base column of each slot
    device_buf<uint32_t> len;         // row lengths
    uint64_t nslices = 0, slots = 0;
    int off_bytes = 4;                // 1, 2 (offsets from the slot base) or 4 (absolute columns)
    bool clustered = false;           // 2-byte offsets as (cluster << 14) | offset, 4 bases per slot
    bool acc_native = false;          // fp32 library: accumulate in fp32 (env SPMV_SLICE_ACC=32)
    double pad_limit = 0.0;           // automatic choice: give up when stored / real entries exceeds it
};

// the row panels of the sweep and the binned layouts (y of one panel fits a workgroup's LDS). The
// one state two layouts share: both cut the same panels, and spmv_hw's streamed copy-back reads
// them for either.
struct panels_state {
    uint64_t npanels = 0;
    uint64_t ent_pad = 0;             // stored entries, panels (sweep) / segments (binned) padded
    uint32_t rmax = 0;                // rows of the largest panel
    device_buf<uint32_t> row;         // first row of each panel [npanels + 1]
};

// panel sweep (kernel 2, sweep.hip; sweep_multi.hip when nvec > 1)
struct sweep_state {
    int variant = 28;                  // sweep-kernel variant (spmv_plan_set_variant)
    uint64_t nunits = 0;               // workgroups of a launch = npanels * split
    uint32_t split = 1;                // > 1: some panel is cut into pieces (partials + combine)
    device_buf<uint32_t> unit_panel;   // panel of each work unit
    device_buf<uint32_t> panel_unit;   // first unit of each panel [npanels + 1]
    device_scratch part;               // split > 1: nunits x (panels.rmax + 1) partial sums (accumulator type)
    double xbias_split = 0.0;          // the pieces' XCC bias in use (split plans; env SPMV_SWEEP_XCC_BIAS)
    device_buf<unsigned long long> steal;  // tools build, split > 1: per unit, iterations claimed
                                           // from the front (low word) and back (high word) by the
                                           // work-stealing variants 37-39; re-armed by k_sweep_combine
    bool can_steal = false;            // the stealing variants can run on this plan (tools build)
    device_buf<uint32_t> panel_cnt;    // split > 1 with env SPMV_SWEEP_COMBINE=fused: per-panel count of
                                       // finished pieces (the last one combines, sweep.hip
                                       // write_panel); null (default): k_sweep_combine
    int acc_bytes = 8;                 // LDS accumulator: 8 (fp64) or 4 (fp32 via CAS, env SPMV_SWEEP_ACC=32)
    int nvec = 1;                      // > 1: spmv_multi's one-pass sweep plan, panels sized for this many
                                       // accumulators per row, unpacked entries, never split; run only by
                                       // launch_sweep_multi (sweep_multi.hip)
    device_buf<uint32_t> col, unit_ent;
    device_buf<uint16_t> row;
    device_buf<ValueType> val;
    device_buf<uint32_t> cbase;      // packed form: base column per 128-entry chunk
    bool packed = false;
    bool lane_order = false;         // packed chunks stored in lane order (k_sweep_lane_order)
    bool det = false;                // env SPMV_SWEEP_DETERMINISTIC=1: ordered LDS adds (k_spmv_sweep_turn)
    // delta-coded columns (default for packed lane-ordered plans, env SPMV_SWEEP_DELTA=0 off): the
    // default kernel streams 11 B/entry fp64 (7 fp32) instead of 12 (8); the 12-byte rc words
    // (col) are freed and rebuilt on demand for the kernels that read them
    // (sweep_materialize_rc: deterministic variants, variant 35, ablations)
    device_buf<uint16_t> row16;      // row in panel per entry (bits 0-14) + bit 8 of its delta (lane order)
    device_buf<uint8_t> d8;          // low 8 bits of the column minus the previous entry's column of
                                     // the same wave instruction (the first from the chunk base)
    device_buf<uint32_t> dbase;      // per chunk: base column, or bit 31 | index into side
    device_buf<uint32_t> side;       // absolute columns (lane order) of chunks with a gap > 511
    uint64_t side_chunks = 0;
    bool delta = false;
    bool wide = false;               // some chunks span >= 65536 columns: their columns live only in
                                     // the side table (delta plans; no 12-byte rc words can be rebuilt)
};

// binned (kernel 6, binned.hip): entries ordered (window, panel), segments padded
struct binned_state {
    uint32_t nwin = 0, W = 0;          // column windows of W columns (x staged in LDS by pass 1)
    uint32_t W1 = 0;                   // width of the odd windows (W: the even ones; XCC bias)
    uint64_t nunits = 0;               // pass-1 work units
    device_buf<ValueType> val;
    device_buf<uint16_t> colw;         // column - window base
    device_scratch rowp;               // u16 row - panel base, or (delta) u8 row deltas
    bool delta = false;                // segments sorted by row, 1-byte deltas (binned.hip)
    bool prod_temporal = false;        // pass 1 stores the products with the default cache policy
                                       // (they stay partly in MALL for pass 2): products <= 1 GiB
    device_scratch prod_alloc;         // the products' allocation
    ValueType *prod = nullptr;         // products, written by pass 1 and read by pass 2: a pointer into
                                       // prod_alloc (it may start past its base), not owned
    device_buf<uint64_t> seg;          // padded segment offsets [nwin * npanels + 1]
    device_buf<uint64_t> seg_hi;       // variants 1 / 2 (tests): seg + seg_base, read by pass 2
    uint64_t seg_base = 0;             // with prod / rowp rebased by -seg_base (same addresses)
    device_buf<uint64_t> ub;           // pass-1 unit boundaries [nunits + 1]
    device_buf<uint32_t> uwin;         // window of each pass-1 unit
    double skew_limit = 0.0;           // automatic choice: give up (rc 2) when a panel holds more than
                                       // this many times the mean entries (long rows: pass 2 would
                                       // serialise their LDS adds on one address)
    double row_limit = 0.0;            // automatic choice: give up (rc 2) when one row holds more than
                                       // this fraction of a panel's mean entries (same reason; env
                                       // SPMV_BIN_ROW_LIMIT overrides the automatic value)
};

// spmv_hw's streamed copy-back (csr_hw_wrapper.cpp): while y_flag is set, the sweep kernel (or
// binned's pass 2) stores y_epoch into y_flag[panel] (host memory) once the panel's rows of y are
// in memory. Both pointers are the wrapper's, lent for one run: never freed here.
struct release_state {
    uint32_t *y_flag = nullptr;
    uint32_t y_epoch = 0;
    ValueType *y_host = nullptr;  // (tools build, SPMV_HW_DIRECT=1) the sweep stores y here instead
                                  // of d_y: mapped pinned host memory
};

// spmv_plan_run_graph (graph.cpp): `iters` SpMVs on (x, y) captured once, replayed per call
struct graph_state {
    hipGraphExec_t exec = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second capture stream (the tools build's "dag" form: the combines)
    const ValueType *x = nullptr;   // the caller's vectors the capture holds (not owned)
    ValueType *y = nullptr;
    int iters = 0;
    device_scratch part2;           // split sweep plans: a second partial buffer beside sweep.part, so
                                    // that step k + 1's sweep can run while step k's partials wait
                                    // for their combine
    device_buf<uint32_t> count;     // "behind" form: two chunk counters
    hipError_t drop_exec()          // a capture made for other vectors, or another variant, must not be replayed
    {
        hipGraphExec_t e = exec;
        exec = nullptr;
        return e ? hipGraphExecDestroy(e) : hipSuccess;
    }
    ~graph_state()  // (not copyable: its buffers are not)
    {
        (void)drop_exec();
        if (stream)
            (void)hipStreamDestroy(stream);
        if (stream2)
            (void)hipStreamDestroy(stream2);
    }
};

// timing (HIP events around the main kernel, on the launch stream)
struct timing_state {
    bool on = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t used = 0;
    timing_state() = default;
    timing_state(const timing_state &) = delete;
    ~timing_state()
    {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
    }
};

}  // namespace spmvhw

// What a plan knows before any layout is built: plan_create_from_slice fills it once, and every
// candidate layout (the tuner's, the automatic slice attempt, the multi-vector sweep) starts
// from a copy.
struct plan_seed {
    int device = 0;
    IndexType nr_rows = 0, nr_cols = 0;
    uint64_t nnz = 0;
    uint64_t nzr = 0;          // non-empty rows
    bool has_empty = false;
    int sweep_threads = spmvhw::kSweepThreads;  // workgroup size: 1024, 512 or 256 (env SPMV_SWEEP_THREADS)
    double locality = -1.0;    // probe result used by the automatic kernel choice
};

// The plan: the seed, which layout it is, and every layout's state (plain members; the unused
// layouts' are a few dozen null words). The members free themselves; the destructor only waits
// for the device to be done with them.
struct spmv_plan : plan_seed {
    spmv_plan() = default;
    explicit spmv_plan(const plan_seed &seed) : plan_seed(seed) {}
    int kernel = 0;
    int op = SPMV_OP_N;        // SPMV_OP_T: the plan holds A^T of the slice it was created from
    int variant = 0;           // variant bits of every layout but the sweep (spmv_plan_set_variant)
    double tuned_ms[4] = {-1.0, -1.0, -1.0, -1.0};  // SPMV_HW_KERNEL=tune: tiles / sweep / slices / binned ms

    spmvhw::tiles_state tiles;
    spmvhw::csr_state csr;
    spmvhw::blocked_state blocked;
    spmvhw::slices_state slices;
    spmvhw::panels_state panels;
    spmvhw::sweep_state sweep;
    spmvhw::binned_state binned;
    spmvhw::release_state release;
    spmvhw::graph_state graph;
    spmvhw::timing_state timing;

    uint64_t device_bytes() const;
    uint64_t algorithmic_bytes() const;
    ~spmv_plan()  // (also on error paths)
    {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

namespace spmvhw {

// Launch, or (warm) only have the runtime load the kernel's code object: plan creation runs the
// launchers warm so that the first SpMV of a plan does not pay the lazy module load (~8 ms).
template <typename K, typename... Args>
inline void launch_or_warm(bool warm, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args)
{
    if (warm) {
        hipFuncAttributes a;
        (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(kernel));
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    }
}

// What a kernel id means to the host (DESIGN.md §3 "The layout table"): one row per kKernel*
// id, defined beside its kernel. A new layout is one new row plus its file. (A row is a constant
// inside its accessor: at namespace scope the device compilation would emit it too, and it
// names host functions.)
struct layout_ops {
    const char *name;         // the SPMV_HW_KERNEL spelling
    const char *trace_label;  // the build's label under SPMV_HW_TRACE
    // 0 ok, 1 error, 2 the layout cannot hold this matrix: an automatic plan takes decline_to
    int (*build)(spmv_plan &p, const IndexType *h_rp, const IndexType *d_col, const ValueType *d_val, hipStream_t s);
    int decline_to;  // -1: none
    // one SpMV: before (may be null), launch -- the main kernel, what the timing events bracket --
    // and after (may be null); only kernels and memsets, so the sequence is capturable
    hipError_t (*before)(const spmv_plan &p, ValueType *d_y, hipStream_t s);
    hipError_t (*launch)(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s);
    hipError_t (*after)(const spmv_plan &p, ValueType *d_y, hipStream_t s);
    void (*warm)(const spmv_plan &p, hipStream_t s);  // loads the code objects of the above, no launch
    uint64_t (*device_bytes)(const spmv_plan &p);
    uint64_t (*units)(const spmv_plan &p);     // spmv_plan_stats.nr_tiles: work units of the main kernel
    uint64_t (*unit_nnz)(const spmv_plan &p);  // spmv_plan_stats.tile_nnz
    uint32_t (*blocks)(const spmv_plan &p);    // spmv_plan_stats.blocks
    int (*format_bits)(const spmv_plan &p);    // the layout's bits of spmv_plan_stats.format
    uint64_t (*stored_entries)(const spmv_plan &p);  // spmv_hw's hw_matrix: entries with padding,
    void *(*index_stream)(const spmv_plan &p);       // and the device array that holds their indices
    int tune_slot;                             // index into spmv_plan::tuned_ms; -1: not a tune candidate
    int product_variants[2];                   // what the product library accepts beside 0 (0: nothing more)
    int (*set_variant)(spmv_plan &p, int variant);  // 0, or 1 with the error set
    bool host_y;                               // the kernel can store y to release.y_host (tools build)
    // the plan as it stands (its variant included) writes y panel by panel and can flag each panel
    // as it is stored (release.y_flag: spmv_hw's streamed copy-back); null: the layout never can
    bool (*flags_panels)(const spmv_plan &p);
};
const layout_ops &tiles_layout(), &gold_layout(), &sweep_layout(), &fpga_layout(), &blocked_layout(), &slices_layout(),
    &binned_layout();
const layout_ops &layout_of(int kernel);  // plan.cpp: the rows by kernel id
constexpr int kKernelCount = 7;
// a launcher with a warm flag as a row's launch and warm entries
using launcher = hipError_t(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm);
template <launcher F>
hipError_t launch_of(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s)
{
    return F(p, d_x, d_y, s, false);
}
template <launcher F>
void warm_of(const spmv_plan &p, hipStream_t s)
{
    (void)F(p, nullptr, nullptr, s, true);
}
inline uint32_t one_block(const spmv_plan &) { return 1; }
inline int set_tile_variant(spmv_plan &p, int variant)  // the tile kernel's two variant bits (every CSR-order row too)
{
    p.variant = variant & 3;
    return 0;
}

// kernels.hip
hipError_t launch_spmv(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false);
hipError_t launch_fixup(const spmv_plan &p, ValueType *d_y, hipStream_t s, bool warm = false);
hipError_t launch_pack(const IndexType *d_col_src, const ValueType *d_val_src, uint64_t nnz,
                       uint64_t nnz_pad, uint32_t ncols, uint32_t *d_col, ValueType *d_val,
                       uint32_t *d_bad, hipStream_t s);
hipError_t launch_validate(const IndexType *d_col, uint64_t nnz, uint32_t ncols, uint32_t *d_bad, hipStream_t s);
// tile column bases (min column of each tile's real entries); *d_maxspan = max over tiles of
// (max column - min column)
hipError_t launch_tile_span(const uint32_t *d_col, uint64_t nnz, uint64_t ntiles, uint32_t *d_cbase,
                            uint32_t *d_maxspan, hipStream_t s);
// up to 4 cluster bases per tile (bases u32[4 ntiles]); *d_bad |= 1 when a tile needs more
hipError_t launch_tile_clusters(const uint32_t *d_col, uint64_t nnz, uint64_t ntiles, uint32_t *d_bases,
                                uint32_t *d_bad, hipStream_t s);
hipError_t launch_cluster_encode(const uint32_t *d_col, uint64_t nnz, uint64_t nnz_pad, const uint32_t *d_bases,
                                 uint16_t *d_out, hipStream_t s);
// col - cbase[tile] as `bytes`-wide offsets (2 or 1)
hipError_t launch_narrow(const uint32_t *d_col, uint64_t nnz, uint64_t nnz_pad, const uint32_t *d_cbase,
                         void *d_out, int bytes, hipStream_t s);

// gold.hip
hipError_t launch_gold(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false);
int fpga_params(spmv_plan &p);  // csr.fpga_vf / csr.fpga_width from env SPMV_FPGA_VF / SPMV_FPGA_BLOCK (kernels 3 and 4)

// blocked.hip
hipError_t launch_blocked(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false);
int build_blocked(spmv_plan &p, const IndexType *h_rp, const IndexType *d_col_src, const ValueType *d_val_src,
                  hipStream_t s);

// slices.hip
hipError_t launch_slices(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false);
int build_slices(spmv_plan &p, const IndexType *h_rp, const IndexType *d_col_src, const ValueType *d_val_src,
                 hipStream_t s);
// K = nvec (2, 4 or 8) right-hand sides in one pass over a slice plan; X and Y row-major
hipError_t launch_slices_multi(const spmv_plan &p, int nvec, const ValueType *d_X, ValueType *d_Y, hipStream_t s,
                               bool warm = false);

// binned.hip
hipError_t launch_binned(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false);
// 0 ok, 1 error, 2 the segment table would be too large (caller may use another kernel)
int build_binned(spmv_plan &p, const IndexType *h_rp, const IndexType *d_col_src, const ValueType *d_val_src,
                 hipStream_t s);

// sweep.hip
// phase 0: the sweep and (split plans) the combine; 1: the sweep only; 2: the combine only.
// part: the partial-sum buffer of a split plan (null: the plan's own sweep.part)
// behind: (spmv_plan_run_graph of a split plan) the previous step's combine, run by extra blocks
// of this sweep launch (sweep.hip, combine_behind); only where sweep_behind_ok
struct sweep_behind {
    const void *cpart = nullptr;  // the previous step's partial sums (null: nothing to combine)
    uint32_t *ccount = nullptr;   // this launch's chunk counter (zero when it starts)
    uint32_t *cnext = nullptr;    // zeroed by this launch: the next launch's counter
    uint32_t blocks = 0;          // extra blocks when cpart is set
    uint32_t rows_per_thread = 4; // a chunk is rows_per_thread x block rows (2, 4 or 8)
};
hipError_t launch_sweep(const spmv_plan &p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool warm = false,
                        int phase = 0, void *part = nullptr, const sweep_behind *behind = nullptr);
bool sweep_behind_ok(const spmv_plan &p);  // the plan's sweep launch can carry a combine behind
// 0 ok, 1 error, 2 the padded layout would overflow 32-bit entry offsets (caller may use tiles)
int build_sweep(spmv_plan &p, const IndexType *h_rp, const IndexType *d_col_src, const ValueType *d_val_src,
                hipStream_t s);
int probe_locality(const IndexType *d_rp, const IndexType *d_col, IndexType n, hipStream_t s, double *frac);
int sweep_materialize_rc(spmv_plan &p);  // delta plan: rebuild the 12-byte rc words (once)

// sweep_multi.hip
// K = nvec (2, 4 or 8) right-hand sides in one pass over a sweep plan built with sweep.nvec = nvec;
// X and Y row-major. Enqueues only the kernel (capturable)
hipError_t launch_sweep_multi(const spmv_plan &p, int nvec, const ValueType *d_X, ValueType *d_Y, hipStream_t s,
                              bool warm = false);

// a kernel over `items` threads in blocks of `block`; the launch's error
template <typename K, typename... Args>
inline hipError_t launch_items(K kernel, uint64_t items, unsigned block, hipStream_t s, Args... args)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)((items + block - 1) / block)), dim3(block), 0, s, args...);
    return hipGetLastError();
}
// compute units of the device (256 when the query fails)
inline int device_cu_count(int device)
{
    hipDeviceProp_t prop;
    return hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0
               ? prop.multiProcessorCount
               : 256;
}

// plan.cpp
constexpr int kKernelTune = -2;
// env SPMV_HW_KERNEL (its only reader): a kernel id by its row's name, kKernelTune for "tune",
// -1 for the automatic choice (unset, "auto", or no row's name)
int requested_kernel();
// Enqueues one SpMV on s by the plan's row: before, launch (between a timing event pair when
// `timing`), after
int run_impl(spmv_plan *p, const ValueType *d_x, ValueType *d_y, hipStream_t s, bool timing);
// the plan's next timing event pair (created on first use), e0 recorded on s
int timing_begin(spmv_plan *p, hipStream_t s, hipEvent_t *e1);

// graph.cpp
// ms per SpMV of a built layout on scratch x / y (SPMV_HW_KERNEL=tune)
int time_layout(spmv_plan &P, const ValueType *d_x, ValueType *d_y, hipStream_t s, double *ms);
int graph_form(const spmv_plan *p);  // how spmv_plan_run_graph captures: 0 serial chain, 1 two-stream DAG, 2 behind

// upload.cpp
int upload_staged(void *dst, const void *src, size_t bytes, hipStream_t s);  // pageable H2D, synchronous
// Fills `out` (spmv_host.hpp) from device arrays: slice_device_args, then hipSetDevice, row_ptr
// copied to the host on `stream`, slice_rebase against nr_nzeros.
int slice_from_device(const char *who, csr_slice &out, const void *handle, int device, IndexType n, IndexType m,
                      IndexType nr_nzeros, const IndexType *d_row_ptr, const IndexType *d_col, const ValueType *d_val,
                      hipStream_t stream);
// The slice's entries on the device: its own pointers, or (host slice) copies uploaded into
// up_col / up_val on the slice's stream
int slice_entries_on_device(const csr_slice &sl, device_scratch &up_col, device_scratch &up_val,
                            const IndexType **d_col, const ValueType **d_val);
// plan.cpp: the plan of the slice (op = SPMV_OP_T: of its device transpose, transpose_slice, the plan's op set).
// force_kernel >= 0: that kernel as if env SPMV_HW_KERNEL named it (spmv_multi's slice path).
// multi_nvec > 1 (spmv_multi's one-pass sweep), with force_kernel = -1: the sweep plan is built
// with that many accumulators per row (sweep.nvec) when the automatic choice for the
// matrix is the sweep or the binned kernel, the unsplit panels fill a round of workgroups and
// the build does not decline -- otherwise the plan is the ordinary one (sweep.nvec = 1), exactly
// as without the argument.
int plan_create_from_slice(spmv_plan **out, int device, int op, const csr_slice &sl, int force_kernel = -1,
                           int multi_nvec = 1);

// transpose.hip
bool bad_op(const char *who, int op);  // true (and the error set) unless op is SPMV_OP_N or SPMV_OP_T
int check_transpose_size(const char *who, uint64_t nnz);  // nonzero (error set) above 2^31 - 1 non-zeros
// A^T of an n x m CSR slice on the device, stable and deterministic. h_rp: the
// slice's row_ptr on the host, rebased to 0 and non-decreasing; d_col / d_val: its entries on the
// device (only read). Writes d_t_rp[m + 1], d_t_col[nnz] (slice-local source rows), d_t_val[nnz];
// returns once the work has completed on s, its temporaries freed.
int csr_transpose_device(IndexType n, IndexType m, const IndexType *h_rp, const IndexType *d_col,
                         const ValueType *d_val, IndexType *d_t_rp, IndexType *d_t_col, ValueType *d_t_val,
                         hipStream_t s);
// A^T of a slice as the creates take it: an m x n device slice whose entries live in the two buffers
struct transposed_csr {
    csr_slice slice;
    device_scratch col, val;
};
// sl's entries on the host (uploaded first) or the device; checks the size limit
int transpose_slice(transposed_csr &t, const csr_slice &sl);

// mgpu.cpp helpers for spmv_hw's RCCL merge (csr_hw_wrapper.cpp): a clique over n distinct
// devices (one rank each, ncclCommInitAll) that borrows the units' plans and takes each device's
// x per run; y of a gather / reduce lands in rank 0's full-length buffer
int mgpu_create_borrowed(spmv_mgpu **out, int n, const int *devices, const IndexType *bounds, IndexType nr_cols,
                         const spmv_plan *const *plans);
int mgpu_run_on(spmv_mgpu *mg, int exchange, const ValueType *const *x_dev);
const ValueType *mgpu_root_y(const spmv_mgpu *mg);
int mgpu_rccl_calls(const spmv_mgpu *mg);  // RCCL calls per step of the last run (run, _pipelined, _graph)
}  // namespace spmvhw

#define SPMV_TRY(expr)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            spmvhw::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));             \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)
// the same inside a plan build and its steps, "<build>: <expr>: <hip error>": the file's kWho names the build
#define SPMV_BUILD_TRY(expr)                                                                          \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            spmvhw::set_error(std::string(kWho) + ": " + #expr + ": " + hipGetErrorString(e_));       \
            return 1;                                                                                 \
        }                                                                                             \
    } while (0)
