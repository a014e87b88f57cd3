// Host-only internals of libspmv_hw (no HIP): what host.cpp, layout.cpp, trsv_plan.cpp and reader.cpp share
// with the rest of the library. tests/sanitize/Makefile compiles host.cpp, layout.cpp and reader.cpp with g++
// -fsanitize=... into a host-only check program (tests/trsv_host does the same for trsv_plan.cpp), so nothing
// here may need the HIP headers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "csr_hw_wrapper.h"

namespace spmvhw {

void set_error(const std::string &msg);
const char *get_error();

// Environment switches of the measurement-only tools build (make ablations, -DSPMV_ABLATIONS:
// layouts and schedules that were measured and not kept, or that tests force). The product
// library reads only the caller-facing knobs INTEGRATION.md §1.4 documents; there this is null.
inline const char *ablation_env(const char *name)
{
#ifdef SPMV_ABLATIONS
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// The rows [row_begin, row_end) of a CSR matrix as every create call takes them:
// filled by slice_from_host, or from device arrays by slice_from_device (spmv_internal.hpp), and
// consumed by plan_create_from_slice, multi_create and transpose_slice.
struct csr_slice {
    IndexType n = 0, m = 0;           // rows of the slice, columns of the matrix
    std::vector<IndexType> rp;        // n + 1 on the host, rp[0] = 0, non-decreasing
    const IndexType *col = nullptr;   // the slice's entries: the caller's arrays offset by the
    const ValueType *val = nullptr;   // slice's first entry (null stays null)
    bool on_device = false;           // where col / val live
    void *stream = nullptr;           // opaque here (a hipStream_t): the stream the creates work on
    uint64_t nnz() const { return rp.empty() ? 0 : rp.back(); }
};

// Fills `out` with rows [row_begin, row_end) of a host matrix. `handle` is the caller's
// out-handle: null is a bad argument like a null matrix or a range outside it
// ("<who>: bad arguments").
int slice_from_host(const char *who, csr_slice &out, const void *handle, const csr_matrix *m, IndexType row_begin,
                    IndexType row_end);
// The null check of a device slice ("<who>: null argument"): the out-handle, and row_ptr unless
// there are no rows. slice_from_device makes it before its first HIP call.
int slice_device_args(const char *who, const void *handle, IndexType n, const IndexType *d_row_ptr);
// The fillers' common end. s.rp holds n + 1 row_ptr entries as the caller has them and s.col /
// s.val the caller's arrays: subtracts rp[0], checks rp[n] against *nr_nzeros when given (the
// message names <who>), offsets col / val and checks that rp does not decrease.
int slice_rebase(const char *who, csr_slice &s, const IndexType *nr_nzeros = nullptr);

// Layout planner of the panel-sweep, binned and tile builds (layout.cpp): the host arithmetic that decides
// a plan's panels, work units, windows, segments and tile tables. Pure functions of their arguments: no HIP and
// no environment -- build_sweep / build_binned read the switches and pass them in.
constexpr uint64_t kSweepLdsBytes = 160 * 1024;       // LDS of one CU holds the panel's y
constexpr uint64_t kSweepChunk = 128;                 // entries per packed chunk (one wave, 2 per lane)
constexpr uint32_t kBinPer = 16 / sizeof(ValueType);  // binned: entries per 16-byte vector
constexpr uint64_t kBinAlign = 128;  // binned, entries: window ranges and pass-1 units start at multiples

// the fewest panels of at most rmax rows that hold n rows
inline uint64_t min_panels(uint64_t n, uint32_t rmax) { return std::max<uint64_t>(1, (n + rmax - 1) / rmax); }
// the most rows of a sweep panel: a workgroup of `threads` gets threads / 1024 of a CU's LDS (less
// 256 B of static LDS) for nvec accumulators of acc_bytes per row and the scratch row; row indices are u16
inline uint32_t sweep_rmax(int threads, uint64_t acc_bytes, int nvec)
{
    const uint64_t lds_bytes = kSweepLdsBytes * threads / 1024 - 256;
    return (uint32_t)std::min<uint64_t>(lds_bytes / (acc_bytes * nvec) - 1, 65534);
}

struct panel_options {
    uint64_t wgs = 256;        // resident workgroups per round: multi-panel cuts are whole rounds
    uint64_t P_first = 1;      // the first panel count to try
    bool allow_split = false;  // split mode (few full-size panels, each cut into pieces) may be chosen,
    bool force_split = false;  // or is whenever at least 2 pieces per panel fit
    uint64_t acc_bytes = 8, val_bytes = sizeof(ValueType);  // split mode's cost test: a partial sum, a value
    double xbias = 0.0;        // even / odd panel bias of the cut (0: even cut)
};
struct panel_cut {
    std::vector<uint32_t> prow;  // first row of each panel, and n
    bool split_mode = false;
    double xbias = 0.0;          // the bias the cut was made with (0 after a fallback to the even cut)
};
// nnz-balanced panels of at most rmax rows: panel q ends at the first row whose start reaches q/P of
// the entries (weighted by the bias), P searched upwards from P_first in whole rounds.
// Returns 0, or 1 with the error "<who>: cannot form panels".
int plan_panels(const char *who, const IndexType *h_rp, IndexType n, uint64_t nnz, uint32_t rmax,
                const panel_options &o, panel_cut &out);

struct sweep_units {
    std::vector<uint32_t> off, poff;  // first entry of each panel: in CSR order, padded to whole chunks
    std::vector<uint32_t> punit;      // first unit of each panel [P + 1]
    std::vector<uint32_t> upanel;     // panel of each unit (one slot when there is none)
    std::vector<uint32_t> uent;       // first padded entry of each unit [U + 1]
    uint32_t rmax_used = 0;           // rows of the largest panel
    uint32_t sweep_split = 1;         // > 1: some panel has several units (combine needed)
    double xbias_split = 0.0;         // the bias the pieces were cut with
};
// The sweep's work units over the panels `prow`: whole chunks of each panel's padded entries, in split
// mode `wgs / P` pieces per panel (pieces_override > 0: that many) cut with the even / odd bias
// `xbias_split`. Outside split mode a panel with more than twice the mean entries is still cut, unless
// whole_panels (multi-vector sweep plans: one unit per panel, always).
// Returns 0, or 2 with the error "<who>: padded entry count exceeds 32 bits".
int plan_sweep_units(const char *who, const IndexType *h_rp, const std::vector<uint32_t> &prow, bool split_mode,
                     uint64_t wgs, int pieces_override, double xbias_split, sweep_units &out,
                     bool whole_panels = false);

// Binned's column windows: nwin of them, at most wmax columns (LDS, u16 offsets), multiples of
// kBinPer, whole rounds of `cus` workgroups where ncols allows. Even windows are W0 wide, odd ones
// W1 (W0 + W1 = 2 W): the bias d widens the even ones to W (1 + d) when nwin is whole rounds and
// both widths fit.
struct bin_windows {
    uint64_t wmax = 0, nwin = 1, W = kBinPer, W0 = kBinPer, W1 = kBinPer;
};
bin_windows plan_bin_windows(uint64_t ncols, uint64_t cus, double d);

// Binned's segments (cnt + esc entries each, padded to kBinPer, every window starting on a kBinAlign
// boundary) and the pass-1 units of whole kBinAlign groups over the non-empty windows.
struct bin_units {
    std::vector<uint64_t> seg;   // padded (window, panel) segment offsets, window-major [nwin P + 1]
    std::vector<uint64_t> ub;    // pass-1 unit boundaries [units + 1]
    std::vector<uint32_t> uwin;  // window of each pass-1 unit
};
void plan_bin_units(const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &esc, uint64_t nwin, uint64_t P,
                    uint64_t cus, bin_units &out);

// The tile build's host arithmetic (layout.cpp; build_tiles uploads the result): the flagged-tile
// representation of spmv_internal.hpp's head comment over tiles of kTileNnz entries.
constexpr int kWave = 64;
constexpr int kLaneEntries = 4;               // entries per lane per wave step
constexpr int kStep = kWave * kLaneEntries;   // 256 entries per wave step
constexpr int kTileSteps = 2;                 // wave steps per tile
constexpr int kTileNnz = kStep * kTileSteps;  // 512 entries per wave tile
struct tile_plan {
    uint64_t nnz_pad = 0, ntiles = 0;  // nnz rounded up to whole tiles
    std::vector<uint32_t> rowend;      // bit k set <=> entry k ends its row [nnz_pad / 32]
    std::vector<uint32_t> tile_info;   // (non-empty rows ended before the tile << 1) | continues a row [ntiles + 1]
    std::vector<uint32_t> row_id;      // the non-empty rows in order; filled only when has_empty
    std::vector<uint32_t> cross;       // (row, first tile, last tile) of every row in more than one tile
};
// Returns 0, or 1 with the error "too many non-empty rows for the tile table" or "internal:
// unterminated row crossing".
int plan_tiles(const IndexType *h_rp, IndexType n, uint64_t nnz, bool has_empty, tile_plan &out);

// Host planner of the sparse triangular solve (trsv_plan.cpp): the dependency levels of
// the `uplo` triangle of a square CSR matrix, the launch list one solve walks, and the permuted layout
// trsv.hip uploads. No HIP and no environment.
constexpr uint32_t kTrsvChainRows = 1024;  // a level of at most this many rows is narrow: runs of narrow
                                           // levels share one single-workgroup launch (one row per thread)
constexpr uint32_t kTrsvLongRow = 32;      // a row with more off-diagonal entries than this gets a whole wave
struct trsv_launch {
    uint32_t chain;                    // 1: k_trsv_chain over levels [level_begin, level_end); 0: k_trsv_level
    uint32_t level_begin, level_end;   // (a wide launch holds exactly one level)
};
struct trsv_plan {
    std::vector<uint32_t> level;      // dependency level of every row [n]
    std::vector<uint32_t> perm;       // the rows sorted by (level, row) [n]
    std::vector<uint32_t> level_ptr;  // first position of each level in perm / order [levels + 1]
    std::vector<uint32_t> order;      // the rows as the kernels take them: by level, inside a level the short
                                      // rows (by row index) and then the long ones (by row index) [n]
    std::vector<uint32_t> long_ptr;   // first position in `order` of each level's long rows [levels]
    std::vector<uint32_t> offdiag;    // in-triangle off-diagonal entries of every row [n]
    std::vector<trsv_launch> launches;
    int64_t missing_diag_row = -1;    // first row (lowest index) without a stored diagonal; -1: none
    int64_t bad_col_row = -1;         // first row holding a column index >= n; -1: none (the plan is valid)
    uint64_t tri_nnz = 0;             // entries the solve uses: off-diagonal ones, and the stored diagonal
                                      // entries unless the diagonal is unit
    uint64_t nr_chain_levels = 0, max_level_rows = 0;
    uint32_t levels() const { return level_ptr.empty() ? 0 : (uint32_t)level_ptr.size() - 1; }
};
// One pass over the rows (ascending for SPMV_TRSV_LOWER, descending for SPMV_TRSV_UPPER): a row without
// in-triangle off-diagonal entries has level 0, any other 1 + the highest level among their columns.
// rp is rebased to 0; the columns of a row need not be sorted and may repeat.
void plan_trsv(IndexType n, const IndexType *rp, const IndexType *col, int uplo, int diag, trsv_plan &out);
// The layout of a valid plan: the off-diagonal triangle as CSR over the positions of plan.order (the
// entries of a row keep their CSR order, columns stay matrix columns = indices into x), and the
// diagonal of each position (duplicates added in CSR order; 1 when the diagonal is unit).
struct trsv_layout {
    std::vector<uint32_t> rp;  // [n + 1]
    std::vector<IndexType> col;
    std::vector<ValueType> val, diag;
};
void build_trsv_layout(IndexType n, const IndexType *rp, const IndexType *col, const ValueType *val, int uplo,
                       int diag, const trsv_plan &plan, trsv_layout &out);

// wall clock in microseconds (util.cpp:3-8)
double timestamp_us();

// One piece of accum_results' '+=' (csr_hw.cpp:1531-1565): dst[i] += src[i] for i < count, once
// the copy that fills src has landed. `ready` is opaque here (the library passes a hipEvent_t):
// host_accumulate hands it to the caller's wait function before reading src.
struct add_part {
    ValueType *dst;
    const ValueType *src;
    uint64_t count;
    void *ready;
};

struct accum_options {
    bool prefault = true;  // map each thread's ranges of dst writable while the copies run
    bool split = true;     // thread t adds the t-th 1/T of every part (false: whole parts t, t+T, ..)
    int threads = 16;      // at most this many threads (1 below 2^18 values in all)
};

// Adds the parts in on up to opts.threads host threads, in part order; wait(ready) returns 0 once
// a part's source is complete (nonzero: error, message in *err; the adds of that thread stop).
// Returns the timestamp_us at which the last part was seen complete; *failed is set when any
// wait failed.
double host_accumulate(const add_part *parts, size_t nparts, int (*wait)(void *ready, std::string *err),
                       const accum_options &opts, bool *failed, std::string *err);

// maps [p, p + count) writable keeping its contents (madvise(MADV_POPULATE_WRITE), else a
// touch per page)
void prefault(ValueType *p, uint64_t count);

}  // namespace spmvhw
