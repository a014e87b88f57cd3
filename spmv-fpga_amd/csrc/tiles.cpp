// Host side of the flagged-tile representation (kernel 0; the kernels are kernels.hip): the build
// and the tiles' row of the layout table.
//
// Roles taken over from the reference's host format builder (csr_hw.cpp):
//   scan_matrix (:7-146)                  -> one pass over row_ptr (plan_tiles, layout.cpp; no
//                                            per-nnz block search)
//   prepare_balanced_hw_matrix (:327-361) -> empty rows become the row_id map
//   hw_matrix_alloc (:151-183)            -> hipMalloc of the plan buffers
//   create_block_matrix +
//   generate_balanced_hw_submatrix (:190-318) -> k_pack on the GPU (O(nnz), coalesced)
#include <cstdlib>

#include "spmv_internal.hpp"

namespace spmvhw {

// Flagged-tile representation: row-end bitmap, tile table (the host planner's, plan_tiles), packed
// col/val, then the narrowest column encoding every tile allows.
static int build_tiles(spmv_plan &p, const IndexType *h_row_ptr, const IndexType *d_col_src,
                       const ValueType *d_val_src, hipStream_t s)
{
    const uint64_t nnz = p.nnz;
    tile_plan t;
    if (plan_tiles(h_row_ptr, p.nr_rows, nnz, p.has_empty, t))
        return 1;
    tiles_state &w = p.tiles;
    w.nnz_pad = t.nnz_pad;
    w.ntiles = t.ntiles;
    w.ncross = t.cross.size() / 3;
    // (an empty array stays null)
    auto alloc = [](auto &buf, uint64_t count) -> hipError_t { return count ? buf.alloc(count) : buf.release(); };
    SPMV_TRY(alloc(w.col, w.nnz_pad));
    SPMV_TRY(alloc(w.val, w.nnz_pad));
    SPMV_TRY(alloc(w.rowend, t.rowend.size()));
    SPMV_TRY(alloc(w.tile_info, t.tile_info.size()));
    SPMV_TRY(alloc(w.head, w.ntiles));
    SPMV_TRY(alloc(w.tail, w.ntiles));
    SPMV_TRY(alloc(w.cross, t.cross.size()));
    if (p.has_empty)
        SPMV_TRY(alloc(w.row_id, t.row_id.size()));
    if (!t.rowend.empty())
        SPMV_TRY(hipMemcpyAsync(w.rowend, t.rowend.data(), t.rowend.size() * 4, hipMemcpyHostToDevice, s));
    SPMV_TRY(hipMemcpyAsync(w.tile_info, t.tile_info.data(), t.tile_info.size() * 4, hipMemcpyHostToDevice, s));
    if (p.has_empty && !t.row_id.empty())
        SPMV_TRY(hipMemcpyAsync(w.row_id, t.row_id.data(), t.row_id.size() * 4, hipMemcpyHostToDevice, s));
    if (!t.cross.empty())
        SPMV_TRY(hipMemcpyAsync(w.cross, t.cross.data(), t.cross.size() * 4, hipMemcpyHostToDevice, s));
    if (w.nnz_pad)
        SPMV_TRY(launch_pack(d_col_src, d_val_src, nnz, w.nnz_pad, p.nr_cols, w.col, w.val, nullptr, s));
    if (const char *xe = ablation_env("SPMV_TILE_XCD"))
        w.xcd = xe[0] == '1';
    // narrow form: 8- or 16-bit column offsets from a per-tile base when every tile allows it
    // (env SPMV_TILE_NARROW: 0 = keep 32-bit columns, 16 = at most 16-bit, default narrowest)
    const char *nenv = ablation_env("SPMV_TILE_NARROW");
    const int narrow_min = !nenv || !*nenv ? 1 : std::atoi(nenv) == 16 ? 2 : std::atoi(nenv) == 0 ? 4 : 1;
    if (w.ntiles && narrow_min < 4) {
        device_buf<uint32_t> d_span;
        SPMV_TRY(w.cbase.alloc(w.ntiles));
        SPMV_TRY(d_span.alloc(1));
        uint32_t span = 0xFFFFFFFFu;
        hipError_t e = hipMemsetAsync(d_span, 0, sizeof(uint32_t), s);
        if (e == hipSuccess)
            e = launch_tile_span(w.col, nnz, w.ntiles, w.cbase, d_span, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(&span, d_span, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        (void)d_span.release();
        SPMV_TRY(e);
        const int cb = span < 256u && narrow_min <= 1 ? 1 : span < 65536u ? 2 : 4;
        if (cb < 4) {
            SPMV_TRY(w.colnar.alloc_bytes(w.nnz_pad * cb));
            SPMV_TRY(launch_narrow(w.col, nnz, w.nnz_pad, w.cbase, w.colnar.p, cb, s));
            SPMV_TRY(hipStreamSynchronize(s));
            SPMV_TRY(w.col.release());
            w.col_bytes = cb;
        } else {
            SPMV_TRY(w.cbase.release());
            // clustered 16-bit columns: up to four narrow column clusters per tile
            const char *cenv = ablation_env("SPMV_TILE_CLUSTER");
            if (!(cenv && cenv[0] == '0')) {
                device_buf<uint32_t> d_bad;
                SPMV_TRY(w.cbase.alloc(w.ntiles * 4));
                SPMV_TRY(d_bad.alloc(1));
                uint32_t bad = 1;
                e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), s);
                if (e == hipSuccess)
                    e = launch_tile_clusters(w.col, nnz, w.ntiles, w.cbase, d_bad, s);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(s);
                (void)d_bad.release();
                SPMV_TRY(e);
                if (!bad) {
                    SPMV_TRY(w.colnar.alloc_bytes(w.nnz_pad * 2));
                    SPMV_TRY(launch_cluster_encode(w.col, nnz, w.nnz_pad, w.cbase, (uint16_t *)w.colnar.p, s));
                    SPMV_TRY(hipStreamSynchronize(s));
                    SPMV_TRY(w.col.release());
                    w.col_bytes = 2;
                    w.clustered = true;
                } else {
                    SPMV_TRY(w.cbase.release());
                }
            }
        }
    }
    // the planner's pageable host vectors go out of scope: make the copies complete first
    SPMV_TRY(hipStreamSynchronize(s));
    return 0;
}

// ---- the tiles' row of the layout table (spmv_internal.hpp layout_ops) ----
// y of the empty rows: the kernel writes only the rows that have entries
static hipError_t tiles_before(const spmv_plan &p, ValueType *d_y, hipStream_t s)
{
    return p.has_empty || p.nnz == 0 ? hipMemsetAsync(d_y, 0, size_t(p.nr_rows) * sizeof(ValueType), s) : hipSuccess;
}

// the rows that cross tile boundaries (k_fixup), outside the timed main kernel
static hipError_t tiles_after(const spmv_plan &p, ValueType *d_y, hipStream_t s) { return launch_fixup(p, d_y, s); }

static void tiles_warm(const spmv_plan &p, hipStream_t s)
{
    (void)launch_spmv(p, nullptr, nullptr, s, true);
    (void)launch_fixup(p, nullptr, s, true);
}

static uint64_t tiles_device_bytes(const spmv_plan &p)
{
    const tiles_state &w = p.tiles;
    return w.nnz_pad * (w.col_bytes + sizeof(ValueType)) + w.nnz_pad / 8 + (w.ntiles + 1) * 4 +
           (w.col_bytes < 4 ? w.ntiles * (w.clustered ? 16 : 4) : 0) +
           (p.has_empty ? p.nzr * 4 : 0) + w.ntiles * 2 * sizeof(ValueType) + w.ncross * 12;
}

static int tiles_format_bits(const spmv_plan &p)
{
    const tiles_state &w = p.tiles;
    return (w.col_bytes < 4 ? 1 : 0) | (w.col_bytes == 1 ? 8 : 0) | (w.clustered ? 16 : 0);
}

const layout_ops &tiles_layout()
{
    static const layout_ops row = {
        "tiles", "build tile layout", build_tiles, -1,
        tiles_before, launch_of<launch_spmv>, tiles_after, tiles_warm,
        tiles_device_bytes,
        [](const spmv_plan &p) -> uint64_t { return p.tiles.ntiles; },  // units
        [](const spmv_plan &) -> uint64_t { return kTileNnz; },   // unit_nnz
        one_block,
        tiles_format_bits,
        [](const spmv_plan &p) -> uint64_t { return p.tiles.nnz_pad; },  // stored_entries
        [](const spmv_plan &p) -> void * { return p.tiles.col_bytes < 4 ? p.tiles.colnar.p : p.tiles.col.p; },  // index_stream
        0, {0, 0}, set_tile_variant, false, nullptr,  // tune_slot, product_variants, set_variant, host_y, flags_panels
    };
    return row;
}

}  // namespace spmvhw
