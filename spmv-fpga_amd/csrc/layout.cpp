// Host-only layout planner of the panel-sweep, binned and tile builds (spmv_host.hpp): panels, the
// sweep's work units, binned's windows, segments and pass-1 units, the tiles' tables. No HIP and no environment; like
// host.cpp it is also built by tests/sanitize/Makefile (host_check layout).
#include <algorithm>
#include <cmath>

#include "spmv_host.hpp"

namespace spmvhw {

// Split mode: when the slice has fewer panels than resident workgroups (a slice of fewer than ~5M
// rows), the panels keep their full LDS size and each is cut into pieces of whole chunks of its
// column-sorted entries (plan_sweep_units; contiguous column ranges, equal entry counts) -- the
// reference's 2-D blocking (row slices x column blocks, csr_hw.cpp:25-76) with the column blocks
// sized by work; k_sweep_combine adds the pieces' partial sums per row in piece order. Otherwise
// panels are rounded to whole rounds of workgroups and each panel is one unit.
// subdivide: a run of (nearly) empty rows longer than a panel that no nnz-balanced cut reaches --
// most often trailing empty rows -- made every P fail (and the search ran on to P = n); after a
// bounded search the cuts are taken at the first P and any panel above the LDS rows is split into
// panels of at most rmax rows.
int plan_panels(const char *who, const IndexType *h_rp, IndexType n, uint64_t nnz, uint32_t rmax,
                const panel_options &o, panel_cut &out)
{
    const uint64_t wgs = o.wgs;
    std::vector<uint32_t> &prow = out.prow;
    double xbias = o.xbias;
    bool split_mode = false, subdivide = false;
    for (uint64_t P = o.P_first;; ++P) {
        {
            // pieces pay when the slice fills at most half the workgroups with full panels and
            // the partial sums (split * n fp64 values, written once and read once by the
            // combine) stay below 0.6x the entry stream. Measured (profiles/): a 1M-row
            // power-law matrix 14 % faster (partials 0.42x the entries), the N = 8 slice of
            // the 10M/160M matrix 18 % (0.33x), a 300K-row matrix 25 % slower (1.4x)
            const uint64_t S = P ? wgs / P : 0;
            split_mode = !subdivide && o.allow_split && S >= 2 && P * S * 10 >= wgs * 9 &&
                         (o.force_split || 2 * S * n * o.acc_bytes * 5 <= 3 * nnz * (4 + o.val_bytes));
        }
        if (!split_mode && P > 1 && P % wgs)
            P = (P + wgs - 1) / wgs * wgs;  // whole rounds of workgroups
        P = std::min<uint64_t>(P, std::max<uint64_t>(n, 1));
        prow.assign(1, 0);
        bool ok = true;
        IndexType r = 0;
        for (uint64_t q = 1; q <= P && ok; ++q) {
            const uint64_t target =
                split_mode || xbias == 0.0
                    ? nnz * q / P
                    : (uint64_t)(double(nnz) * (double(q) - xbias * double(q & 1)) / (double(P) - xbias * double(P & 1)));
            IndexType e = (q == P) ? n : (IndexType)(std::lower_bound(h_rp, h_rp + n + 1, (IndexType)target) - h_rp);
            e = std::max(e, r);
            if (e - r > rmax && xbias != 0.0 && !split_mode && q < P)
                e = r + rmax;  // a biased cut past the LDS rows: this panel takes what fits
            if (e - r > rmax && subdivide)
                for (; e - r > rmax; r += rmax)
                    prow.push_back(r + rmax);
            if (e - r > rmax)
                ok = false;
            prow.push_back(e);
            r = e;
        }
        if (ok)
            break;
        if (xbias != 0.0 && !split_mode) {  // the biased cut overflows a panel: cut evenly
            xbias = 0.0;
            --P;
            continue;
        }
        if (P >= n || P > 8 * std::max<uint64_t>(min_panels(n, rmax), wgs)) {
            if (subdivide) {
                set_error(std::string(who) + ": cannot form panels");
                return 1;
            }
            subdivide = true;
            xbias = 0.0;
            P = o.P_first - 1;  // (++P)
        }
    }
    out.split_mode = split_mode;
    out.xbias = xbias;
    return 0;
}

// The pieces of every panel: whole chunks, cut with the even / odd XCC bias d (the weight of
// units [0, u) is u - d (u & 1): the units block-round-robin dispatch sends to even XCCs get
// (1 - d) x the mean, the odd ones (1 + d) x); d = 0 cuts evenly
static void cut_units(const std::vector<uint32_t> &poff, const std::vector<uint32_t> &punit, double d,
                      std::vector<uint32_t> &uent)
{
    const uint32_t P = (uint32_t)punit.size() - 1, U = punit[P];
    uent.assign((size_t)U + 1, 0);
    auto wc = [&](uint32_t u) { return double(u) - d * double(u & 1); };
    for (uint32_t q = 0; q < P; ++q) {
        const uint64_t chunks = (uint64_t(poff[q + 1]) - poff[q]) / kSweepChunk;
        const uint32_t k = punit[q + 1] - punit[q], u0 = punit[q];
        for (uint32_t t = 0; t < k; ++t) {
            const uint64_t c = d != 0.0 ? (uint64_t)(double(chunks) * (wc(u0 + t) - wc(u0)) / (wc(u0 + k) - wc(u0)))
                                        : chunks * t / k;
            uent[u0 + t] = (uint32_t)(poff[q] + kSweepChunk * c);
        }
    }
    uent[U] = poff[P];
}

int plan_sweep_units(const char *who, const IndexType *h_rp, const std::vector<uint32_t> &prow, bool split_mode,
                     uint64_t wgs, int pieces_override, double xbias_split, sweep_units &out, bool whole_panels)
{
    const uint32_t P = (uint32_t)(prow.size() - 1);
    std::vector<uint32_t> &off = out.off, &poff = out.poff, &punit = out.punit, &upanel = out.upanel;
    off.assign((size_t)P + 1, 0);
    poff.assign((size_t)P + 1, 0);
    out.rmax_used = 0;
    uint64_t padded = 0;
    for (uint32_t q = 0; q < P; ++q) {
        const uint64_t cnt = uint64_t(h_rp[prow[q + 1]]) - h_rp[prow[q]];
        padded += (cnt + kSweepChunk - 1) / kSweepChunk * kSweepChunk;
        off[q + 1] = (uint32_t)(off[q] + cnt);
        poff[q + 1] = (uint32_t)padded;
        out.rmax_used = std::max(out.rmax_used, prow[q + 1] - prow[q]);
    }
    if (padded > 0xFFFFFFFFull) {  // panel_ent is u32: the padded layout must fit (nnz near 2^32)
        set_error(std::string(who) + ": padded entry count exceeds 32 bits");
        return 2;
    }
    // work units: pieces of whole chunks per panel. split mode: `split` pieces each; any panel
    // with more than twice the mean entry count (a panel holding very long rows) is cut
    // further, so that no workgroup gets more than ~2x the mean work
    uint32_t split = split_mode ? std::max<uint32_t>(1, (uint32_t)(wgs / P)) : 1;
    if (split_mode && pieces_override > 0)
        split = (uint32_t)pieces_override;
    const double mean = P ? double(padded) / P : 0.0;
    punit.assign((size_t)P + 1, 0);
    for (uint32_t q = 0; q < P; ++q) {
        const uint64_t chunks = (uint64_t(poff[q + 1]) - poff[q]) / kSweepChunk;
        uint64_t k = split * std::max<uint64_t>(
                                 1, (uint64_t)std::ceil(double(poff[q + 1] - poff[q]) / std::max(2.0 * mean, 1.0)));
        k = whole_panels ? 1 : std::max<uint64_t>(1, std::min<uint64_t>(k, chunks));
        punit[q + 1] = punit[q] + (uint32_t)k;
    }
    upanel.assign(std::max<uint32_t>(punit[P], 1), 0);
    bool multi = false;
    for (uint32_t q = 0; q < P; ++q) {
        multi |= punit[q + 1] - punit[q] > 1;
        for (uint32_t u = punit[q]; u < punit[q + 1]; ++u)
            upanel[u] = q;
    }
    out.xbias_split = split_mode ? xbias_split : 0.0;
    cut_units(poff, punit, out.xbias_split, out.uent);
    out.sweep_split = multi ? std::max<uint32_t>(split, 2) : 1;
    return 0;
}

bin_windows plan_bin_windows(uint64_t ncols, uint64_t cus, double d)
{
    constexpr uint64_t PER = kBinPer;
    bin_windows w;
    // windows: W <= what 160 KiB of LDS holds (and the u16 offsets), a multiple of PER
    const uint64_t wmax = w.wmax = std::min<uint64_t>((kSweepLdsBytes - 256) / sizeof(ValueType) / PER * PER, 65536);
    uint64_t &nwin = w.nwin, &W = w.W, &W0 = w.W0, &W1 = w.W1;
    if (ncols) {
        const uint64_t rounds = std::max<uint64_t>(1, (ncols + cus * wmax - 1) / (cus * wmax));
        nwin = std::min<uint64_t>(cus * rounds, (ncols + PER - 1) / PER);
        W = ((ncols + nwin - 1) / nwin + PER - 1) / PER * PER;
        nwin = (ncols + W - 1) / W;
    }
    W0 = W1 = W;
    if (!(d > -0.25 && d < 0.25) || nwin < cus || nwin % cus)
        d = 0.0;
    const uint64_t w0 = std::min<uint64_t>(wmax, (uint64_t(std::llround(W * (1.0 + d))) + PER / 2) / PER * PER);
    if (d != 0.0 && w0 >= PER && w0 < 2 * W) {
        W0 = w0;
        W1 = 2 * W - w0;
        if (W1 > wmax) {  // a negative bias past the LDS: even widths
            W0 = W1 = W;
        }
        const uint64_t pw = W0 + W1, k = ncols / pw, rem = ncols - k * pw;
        nwin = 2 * k + (rem == 0 ? 0 : rem <= W0 ? 1 : 2);
    }
    return w;
}

void plan_bin_units(const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &esc, uint64_t nwin, uint64_t P,
                    uint64_t cus, bin_units &out)
{
    constexpr uint64_t PER = kBinPer;
    const uint64_t nseg = nwin * P;
    // padded segment offsets (window-major), then the pass-1 units
    // Each window's range also starts on a 128-entry boundary (the last segment of the window
    // takes the extra pad entries): pass 1's 1-KiB wave loads and stores then cover whole
    // 128-byte lines instead of straddling them (partial-line stores).
    std::vector<uint64_t> &seg = out.seg, &ub = out.ub;
    seg.assign(nseg + 1, 0);
    for (uint64_t k = 0; k < nseg; ++k) {
        seg[k + 1] = seg[k] + (uint64_t(cnt[k]) + esc[k] + PER - 1) / PER * PER;
        if ((k + 1) % P == 0)
            seg[k + 1] = (seg[k + 1] + kBinAlign - 1) / kBinAlign * kBinAlign;
    }
    const uint64_t ent_pad = seg[nseg];
    ub.assign(1, 0);
    out.uwin.clear();
    const double mean = nwin ? double(ent_pad) / double(nwin) : 0.0;
    const uint64_t fill = nwin < cus ? (cus + nwin - 1) / nwin : 1;  // few windows: pieces
    for (uint64_t w = 0; w < nwin; ++w) {
        const uint64_t a = seg[w * P], b = seg[(w + 1) * P], e = b - a;
        if (!e)
            continue;
        uint64_t k = std::max<uint64_t>(fill, (uint64_t)std::ceil(double(e) / std::max(2.0 * mean, 1.0)));
        k = std::max<uint64_t>(1, std::min<uint64_t>(k, e / kBinAlign));  // e: whole 128-entry groups
        ub.back() = a;
        for (uint64_t t = 1; t <= k; ++t) {
            ub.push_back(a + (e / kBinAlign) * t / k * kBinAlign);
            out.uwin.push_back((uint32_t)w);
        }
    }
}

int plan_tiles(const IndexType *h_rp, IndexType n, uint64_t nnz, bool has_empty, tile_plan &out)
{
    out.nnz_pad = (nnz + kTileNnz - 1) / kTileNnz * kTileNnz;
    const uint64_t ntiles = out.ntiles = out.nnz_pad / kTileNnz;
    std::vector<uint32_t> &rowend = out.rowend, &tile_info = out.tile_info, &cross = out.cross;
    rowend.assign(out.nnz_pad / 32, 0u);
    out.row_id.clear();
    for (IndexType r = 0; r < n; ++r) {
        if (h_rp[r + 1] > h_rp[r]) {
            const uint64_t e = h_rp[r + 1] - 1ull;
            rowend[e >> 5] |= 1u << (e & 31);
            if (has_empty)
                out.row_id.push_back(r);
        }
    }
    auto bit = [&](uint64_t k) { return (rowend[k >> 5] >> (k & 31)) & 1u; };
    tile_info.assign(ntiles + 1, 0u);
    uint64_t rr = 0, c = 0;
    for (uint64_t t = 0; t <= ntiles; ++t) {
        const uint64_t k = t * kTileNnz;
        while (rr < n && h_rp[rr + 1] <= k) {
            if (h_rp[rr + 1] > h_rp[rr])
                ++c;
            ++rr;
        }
        if (c > 0x7FFFFFFFull) {
            set_error("too many non-empty rows for the tile table");
            return 1;
        }
        const bool cont = k > 0 && k < nnz && !bit(k - 1);
        tile_info[t] = (uint32_t)(c << 1) | (cont ? 1u : 0u);
    }
    // rows crossing tile boundaries (structural): tile t "has a tail" when its last entry is not
    // a row end and entries follow; a crossing starts at a tile with a tail whose row began in
    // it, and ends at the next tile that contains a row end
    cross.clear();
    std::vector<uint8_t> has_tail(ntiles, 0), has_end(ntiles, 0);
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t w0 = t * (kTileNnz / 32);
        for (uint64_t w = 0; w < kTileNnz / 32; ++w)
            has_end[t] |= rowend[w0 + w] != 0;
        const uint64_t last = (t + 1) * kTileNnz - 1;
        has_tail[t] = (last + 1 < nnz) && !bit(last);
    }
    for (uint64_t t = 0; t < ntiles; ++t) {
        if (!has_tail[t] || !(has_end[t] || t == 0 || !has_tail[t - 1]))
            continue;
        uint64_t j = t + 1;
        while (j < ntiles && !has_end[j])
            ++j;
        if (j >= ntiles) {
            set_error("internal: unterminated row crossing");
            return 1;
        }
        cross.push_back(tile_info[t + 1] >> 1);
        cross.push_back((uint32_t)t);
        cross.push_back((uint32_t)j);
    }
    return 0;
}

}  // namespace spmvhw
