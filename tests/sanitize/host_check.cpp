// Host-only check program for the sanitizer builds (tests/sanitize/Makefile): drives the host
// code of libspmv_hw -- the multi-threaded reader (reader.cpp), the row partition, the exchange
// schedule, the threaded accum_results '+=' (host.cpp), the layout planner (layout.cpp), verification
// and storage_overhead --
// compiled with g++ under AddressSanitizer + UBSan and under ThreadSanitizer. No HIP.
//
//   host_check read <file.mtx> <out.bin>   spmv_read_csr -> binary dump (n, m, nnz, row_ptr, col, val)
//                                          and the header/matrix pair of calls, compared
//   host_check partition                   random row_ptr, 1..16 units, against a restated S1 rule
//   host_check slice                       slice_from_host on whole, empty, last-row and random ranges
//   host_check layout                      the sweep / binned layout planner (layout.cpp): invariants of
//                                          panels, units, windows and segments; pinned edge cases
//   host_check tiles                       the tile planner (layout.cpp plan_tiles): bitmap, tile table, row map
//                                          and crossings against a per-entry recomputation; pinned edge cases
//   host_check schedule                    every exchange at 1..8 ranks, rows covered once
//   host_check accumulate                  producer threads land parts while 16 threads add them
//   host_check verify                      verification / storage_overhead semantics
// Prints "OK <what>" and exits 0; any failed check prints "FAIL ..." and exits 1.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "spmv_host.hpp"

using namespace spmvhw;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static int cmd_read(const char *path, const char *out)
{
    csr_matrix m;
    const int rc = spmv_read_csr(path, &m);
    if (rc) {
        std::printf("READ_ERROR %d %s\n", rc, spmv_hw_last_error());
        return 0;  // an error code is a result too (the caller compares it)
    }
    // the two-call form (csr.cpp's read_csr_header + read_csr_matrix) gives the same arrays
    csr_header h;
    CHECK(spmv_read_csr_header(&h, path) == 0);
    CHECK(h.nr_rows == m.nr_rows && h.nr_cols == m.nr_cols && h.nr_nzeros == m.nr_nzeros);
    csr_matrix m2;
    std::memset(&m2, 0, sizeof(m2));
    m2.nr_rows = h.nr_rows;
    m2.nr_cols = h.nr_cols;
    m2.nr_nzeros = h.nr_nzeros;
    std::vector<IndexType> rp(size_t(h.nr_rows) + 1), ci(std::max<size_t>(h.nr_nzeros, 1));
    std::vector<ValueType> va(std::max<size_t>(h.nr_nzeros, 1));
    m2.row_ptr = rp.data();
    m2.col_ind = ci.data();
    m2.values = va.data();
    CHECK(spmv_read_csr_matrix(&m2, path) == 0);
    CHECK(std::memcmp(rp.data(), m.row_ptr, rp.size() * sizeof(IndexType)) == 0);
    CHECK(std::memcmp(ci.data(), m.col_ind, size_t(h.nr_nzeros) * sizeof(IndexType)) == 0);
    CHECK(std::memcmp(va.data(), m.values, size_t(h.nr_nzeros) * sizeof(ValueType)) == 0);
    FILE *f = std::fopen(out, "wb");
    CHECK(f);
    const uint64_t head[4] = {m.nr_rows, m.nr_cols, m.nr_nzeros, sizeof(ValueType)};
    CHECK(std::fwrite(head, sizeof(head), 1, f) == 1);
    CHECK(std::fwrite(m.row_ptr, sizeof(IndexType), size_t(m.nr_rows) + 1, f) == size_t(m.nr_rows) + 1);
    if (m.nr_nzeros) {
        CHECK(std::fwrite(m.col_ind, sizeof(IndexType), m.nr_nzeros, f) == m.nr_nzeros);
        CHECK(std::fwrite(m.values, sizeof(ValueType), m.nr_nzeros, f) == m.nr_nzeros);
    }
    std::fclose(f);
    spmv_free_csr(&m);
    std::printf("OK read %s\n", path);
    return 0;
}

static int cmd_partition()
{
    std::mt19937_64 g(5);
    for (int it = 0; it < 300; ++it) {
        const uint32_t n = it % 10 == 0 ? 0 : uint32_t(g() % 5000);
        std::vector<IndexType> rp(size_t(n) + 1, 0);
        const uint64_t base = it % 3 == 0 ? 1000 : 0;  // a slice of a larger matrix starts past 0
        rp[0] = (IndexType)base;
        for (uint32_t i = 0; i < n; ++i)
            rp[i + 1] = rp[i] + (IndexType)(g() % 7 == 0 ? g() % 400 : g() % 6);
        for (int units = 1; units <= 16; ++units) {
            std::vector<IndexType> b(units + 1, 0xdeadbeef);
            CHECK(spmv_partition_rows(rp.data(), n, units, b.data()) == 0);
            CHECK(b[0] == 0 && b[units] == n);
            const uint64_t nnz = rp[n] - rp[0];
            for (int u = 1; u < units; ++u) {
                CHECK(b[u] >= b[u - 1]);
                // restated S1 rule: the first row whose start reaches u/units of the non-zeros
                const uint64_t target = rp[0] + nnz * uint64_t(u) / uint64_t(units);
                uint32_t want = 0;
                while (want < n && rp[want] < target)
                    ++want;
                CHECK(b[u] == std::max<IndexType>(want, b[u - 1]));
            }
        }
    }
    IndexType one[2];
    CHECK(spmv_partition_rows(nullptr, 0, 1, one) == 1);
    CHECK(std::strlen(spmv_hw_last_error()) > 0);
    std::printf("OK partition\n");
    return 0;
}

// slice_from_host on one range of a matrix whose arrays are allocated at their exact sizes (a read
// past row_ptr[row_end] is a heap overflow), against the rebased row_ptr computed here
static void check_slice(const IndexType *rp, const IndexType *col, const ValueType *val, IndexType nr_rows,
                        IndexType nr_cols, IndexType b, IndexType e)
{
    csr_matrix m;
    std::memset(&m, 0, sizeof(m));
    m.row_ptr = const_cast<IndexType *>(rp);
    m.col_ind = const_cast<IndexType *>(col);
    m.values = const_cast<ValueType *>(val);
    m.nr_rows = nr_rows;
    m.nr_cols = nr_cols;
    m.nr_nzeros = rp[nr_rows];
    int handle = 0;
    csr_slice s;
    CHECK(slice_from_host("check", s, &handle, &m, b, e) == 0);
    const IndexType n = e - b, base = rp[b];
    CHECK(s.n == n && s.m == nr_cols && !s.on_device && s.stream == nullptr);
    CHECK(s.rp.size() == size_t(n) + 1);
    CHECK(s.rp[0] == 0 && s.rp[n] == rp[e] - rp[b] && s.nnz() == uint64_t(rp[e] - rp[b]));
    for (IndexType r = 0; r <= n; ++r)
        CHECK(s.rp[r] == rp[b + r] - base);
    CHECK(s.col == col + base && s.val == val + base);
}

static int cmd_slice()
{
    std::mt19937_64 g(11);
    for (int it = 0; it < 200; ++it) {
        const IndexType n = 1 + IndexType(g() % 300), ncols = 1 + IndexType(g() % 200);
        // exact-size heap arrays: no vector capacity behind the last element
        IndexType *rp = new IndexType[size_t(n) + 1];
        rp[0] = 0;
        for (IndexType r = 0; r < n; ++r)
            rp[r + 1] = rp[r] + (g() % 3 == 0 ? 0 : IndexType(g() % 9));  // a third of the rows empty
        const IndexType nnz = rp[n];
        IndexType *col = new IndexType[nnz];
        ValueType *val = new ValueType[nnz];
        for (IndexType k = 0; k < nnz; ++k) {
            col[k] = IndexType(g() % ncols);
            val[k] = ValueType(int(g() % 64)) / 8;
        }
        check_slice(rp, col, val, n, ncols, 0, n);      // the whole matrix
        check_slice(rp, col, val, n, ncols, 0, 0);      // empty, at the front
        check_slice(rp, col, val, n, ncols, n, n);      // empty, at row_ptr's last entry
        check_slice(rp, col, val, n, ncols, n - 1, n);  // the last row alone
        // a range that starts and ends on empty rows (when the matrix has two)
        IndexType e0 = n, e1 = n;
        for (IndexType r = 0; r < n; ++r)
            if (rp[r + 1] == rp[r]) {
                if (e0 == n)
                    e0 = r;
                e1 = r;
            }
        if (e0 < e1)
            check_slice(rp, col, val, n, ncols, e0, e1 + 1);
        for (int k = 0; k < 8; ++k) {
            const IndexType b = IndexType(g() % (size_t(n) + 1)), e = b + IndexType(g() % (size_t(n) - b + 1));
            check_slice(rp, col, val, n, ncols, b, e);
        }
        delete[] rp;
        delete[] col;
        delete[] val;
    }
    {
        // every entry lies before row_begin: base == nnz, col / val one past their arrays' end
        const IndexType rp[5] = {0, 3, 5, 5, 5};
        IndexType *col = new IndexType[5]{0, 1, 2, 0, 1};
        ValueType *val = new ValueType[5]{1, 2, 3, 4, 5};
        check_slice(rp, col, val, 4, 3, 2, 4);
        check_slice(rp, col, val, 4, 3, 4, 4);
        // the argument errors
        csr_matrix m;
        std::memset(&m, 0, sizeof(m));
        m.row_ptr = const_cast<IndexType *>(rp);
        m.col_ind = col;
        m.values = val;
        m.nr_rows = 4;
        m.nr_cols = 3;
        m.nr_nzeros = 5;
        int handle = 0;
        csr_slice s;
        CHECK(slice_from_host("who", s, &handle, nullptr, 0, 0) != 0);
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: bad arguments"));
        set_error("");
        CHECK(slice_from_host("who", s, &handle, &m, 3, 2) != 0);
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: bad arguments"));
        set_error("");
        CHECK(slice_from_host("who", s, &handle, &m, 0, 5) != 0);
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: bad arguments"));
        set_error("");
        CHECK(slice_from_host("who", s, nullptr, &m, 0, 4) != 0);  // no out-handle
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: bad arguments"));
        // a row_ptr that decreases inside the range is refused, outside it not looked at
        const IndexType dec[5] = {0, 3, 2, 4, 4};
        m.row_ptr = const_cast<IndexType *>(dec);
        m.nr_nzeros = 4;
        CHECK(slice_from_host("who", s, &handle, &m, 0, 4) != 0);
        CHECK(std::strstr(spmv_hw_last_error(), "row_ptr is not non-decreasing at row 1"));
        CHECK(slice_from_host("who", s, &handle, &m, 2, 4) == 0 && s.nnz() == 2);
        // the device slice's null check, as far as it runs without a device
        CHECK(slice_device_args("who", nullptr, 0, nullptr) != 0);
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: null argument"));
        CHECK(slice_device_args("who", &handle, 4, nullptr) != 0);
        CHECK(slice_device_args("who", &handle, 0, nullptr) == 0);
        CHECK(slice_device_args("who", &handle, 4, rp) == 0);
        // the fillers' common end as slice_from_device uses it: nr_nzeros must match
        const IndexType col12[12] = {};
        csr_slice d;
        d.n = 2;
        d.rp = {7, 9, 12};
        d.col = col12;
        IndexType z = 5;
        CHECK(slice_rebase("who", d, &z) == 0 && d.rp[0] == 0 && d.rp[2] == 5 && d.col == col12 + 7 && !d.val);
        d.rp = {7, 9, 12};
        z = 4;
        CHECK(slice_rebase("who", d, &z) != 0);
        CHECK(!std::strcmp(spmv_hw_last_error(), "who: row_ptr[n]-row_ptr[0] != nr_nzeros"));
        delete[] col;
        delete[] val;
    }
    std::printf("OK slice\n");
    return 0;
}

// ---- the layout planner (layout.cpp): invariants of its results, restated here, not its code ----

static std::vector<IndexType> row_ptr_of(const std::vector<uint32_t> &len)
{
    std::vector<IndexType> rp(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i)
        rp[i + 1] = rp[i] + len[i];
    return rp;
}

// what every panel cut must satisfy; even_cut: also the restated nnz-balanced rule (the caller
// knows that the cut is unbiased and that the search cannot have subdivided)
static void check_panels(const std::vector<IndexType> &rp, uint32_t rmax, const panel_options &o, const panel_cut &c,
                         bool even_cut)
{
    const IndexType n = IndexType(rp.size() - 1);
    const uint64_t nnz = rp[n], P = c.prow.size() - 1;
    CHECK(c.prow.size() >= 2 && c.prow[0] == 0 && c.prow.back() == n);
    for (uint64_t q = 0; q < P; ++q) {
        CHECK(c.prow[q + 1] >= c.prow[q]);
        CHECK(c.prow[q + 1] - c.prow[q] <= rmax);
    }
    CHECK(o.allow_split || !c.split_mode);
    if (!even_cut)
        return;
    if (!c.split_mode && P > 1)
        CHECK(P % o.wgs == 0 || P == n);  // whole rounds of workgroups
    uint32_t want = 0;
    for (uint64_t q = 1; q < P; ++q) {  // the first row whose start reaches q/P of the entries
        const uint64_t target = nnz * q / P;
        while (want < n && rp[want] < target)
            ++want;
        CHECK(c.prow[q] == want);
    }
}

static void check_units(const std::vector<IndexType> &rp, const panel_cut &c, const sweep_units &u)
{
    const uint32_t P = uint32_t(c.prow.size() - 1);
    CHECK(u.off.size() == P + 1u && u.poff.size() == P + 1u && u.punit.size() == P + 1u);
    CHECK(u.off[0] == 0 && u.poff[0] == 0 && u.punit[0] == 0);
    const uint32_t U = u.punit[P];
    CHECK(u.uent.size() == U + 1u && u.upanel.size() == std::max<uint32_t>(U, 1));
    uint32_t rows = 0;
    bool multi = false;
    for (uint32_t q = 0; q < P; ++q) {
        const uint64_t cnt = uint64_t(rp[c.prow[q + 1]]) - rp[c.prow[q]];
        CHECK(u.off[q] == rp[c.prow[q]] && u.off[q + 1] - u.off[q] == cnt);
        CHECK(u.poff[q + 1] - u.poff[q] == (cnt + 127) / 128 * 128);
        const uint64_t chunks = (u.poff[q + 1] - u.poff[q]) / 128, k = u.punit[q + 1] - u.punit[q];
        CHECK(u.punit[q + 1] > u.punit[q]);  // at least one unit (also for a panel without entries)
        CHECK(k <= std::max<uint64_t>(chunks, 1));
        CHECK(u.uent[u.punit[q]] == u.poff[q]);
        for (uint32_t t = u.punit[q]; t < u.punit[q + 1]; ++t)
            CHECK(u.upanel[t] == q);
        rows = std::max(rows, c.prow[q + 1] - c.prow[q]);
        multi |= k > 1;
    }
    CHECK(u.uent[U] == u.poff[P] && u.rmax_used == rows);
    for (uint32_t t = 0; t < U; ++t)
        CHECK(u.uent[t + 1] >= u.uent[t] && u.uent[t] % 128 == 0);
    CHECK((u.sweep_split > 1) == multi);
    CHECK(c.split_mode || u.xbias_split == 0.0);
}

static void check_windows(uint64_t ncols, uint64_t cus, double d)
{
    const bin_windows w = plan_bin_windows(ncols, cus, d);
    CHECK(w.nwin >= 1 && w.W0 + w.W1 == 2 * w.W);
    for (uint64_t x : {w.W, w.W0, w.W1})
        CHECK(x >= kBinPer && x <= w.wmax && x % kBinPer == 0);
    CHECK(d != 0.0 || w.W0 == w.W1);
    if (!ncols)
        return;
    // even windows W0 wide, odd ones W1: the last one starts inside [0, ncols) and ends at or past it
    auto start = [&](uint64_t k) { return k / 2 * (w.W0 + w.W1) + (k & 1 ? w.W0 : 0); };
    CHECK(start(w.nwin - 1) < ncols && start(w.nwin) >= ncols);
}

static void check_bin_units(const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &esc, uint64_t nwin, uint64_t P,
                            uint64_t cus)
{
    bin_units b;
    plan_bin_units(cnt, esc, nwin, P, cus, b);
    const uint64_t nseg = nwin * P;
    CHECK(b.seg.size() == nseg + 1 && b.seg[0] == 0 && b.ub.size() == b.uwin.size() + 1);
    for (uint64_t k = 0; k < nseg; ++k) {
        CHECK(b.seg[k + 1] >= b.seg[k] + cnt[k] + esc[k]);  // monotone, and room for the segment
        CHECK(b.seg[k + 1] % kBinPer == 0);
    }
    for (uint64_t w = 0; w <= nwin; ++w)
        CHECK(b.seg[w * P] % kBinAlign == 0);
    // the units of every non-empty window, in window order, tile the window's range once
    size_t u = 0;
    for (uint64_t w = 0; w < nwin; ++w) {
        const uint64_t a = b.seg[w * P], e = b.seg[(w + 1) * P];
        if (a == e)
            continue;
        CHECK(u < b.uwin.size() && b.uwin[u] == w && b.ub[u] == a);
        for (; u < b.uwin.size() && b.uwin[u] == w; ++u)
            CHECK(b.ub[u + 1] >= b.ub[u] && b.ub[u + 1] <= e && b.ub[u] % kBinAlign == 0);
        CHECK(b.ub[u] == e);  // also the next non-empty window's start: empty ones take no room
    }
    CHECK(u == b.uwin.size());
}

// sweep (bias, split options) and binned (its first P, no split, no bias) on one row_ptr
static void check_layout(const std::vector<IndexType> &rp, uint32_t rmax, uint64_t wgs, double bias, int split,
                         int pieces, bool no_subdivide)
{
    const IndexType n = IndexType(rp.size() - 1);
    const uint64_t nnz = rp[n];
    panel_options o;
    o.wgs = wgs;
    o.P_first = min_panels(n, rmax);
    o.allow_split = split != 0;
    o.force_split = split == 2;
    o.xbias = bias;
    panel_cut c;
    set_error("");
    CHECK(plan_panels("sweep", rp.data(), n, nnz, rmax, o, c) == 0);  // "cannot form panels": never
    CHECK(bias != 0.0 || c.xbias == 0.0);
    check_panels(rp, rmax, o, c, no_subdivide && (c.split_mode || c.xbias == 0.0));
    sweep_units u;
    CHECK(plan_sweep_units("sweep", rp.data(), c.prow, c.split_mode, wgs, pieces, bias, u) == 0);
    check_units(rp, c, u);
    panel_options b;
    b.wgs = wgs;
    b.P_first = std::max<uint64_t>(min_panels(n, rmax), std::min<uint64_t>(wgs, n));
    panel_cut cb;
    CHECK(plan_panels("binned", rp.data(), n, nnz, rmax, b, cb) == 0);
    check_panels(rp, rmax, b, cb, no_subdivide);
    CHECK(!std::strlen(get_error()));
}

static int cmd_layout()
{
    std::mt19937_64 g(17);
    const uint64_t wgss[] = {64, 256, 304};
    const double biases[] = {0.0, 0.015, -0.02, 0.1, 0.49};
    for (int it = 0; it < 400; ++it) {
        // rows of 1..4 entries and rmax = 64: a panel cut at P holds fewer than nnz / P + 5 rows,
        // so the search ends by P = 4 n / 59 -- inside its bound of 8 max(n / 64, wgs) and below
        // P = n -- and never subdivides; the even cut's restated rule then holds
        const bool plain = it % 2 == 0;
        std::vector<uint32_t> len(it % 25 == 0 ? g() % 3 : g() % 4000);
        for (auto &l : len)
            l = plain ? 1 + uint32_t(g() % 4) : g() % 9 == 0 ? uint32_t(g() % 3000) : uint32_t(g() % 40 == 0 ? g() % 6 : 0);
        const std::vector<IndexType> rp = row_ptr_of(len);
        for (int k = 0; k < 3; ++k)
            check_layout(rp, plain ? 64 : (g() % 2 ? 7 : 300), wgss[g() % 3], biases[g() % 5], int(g() % 3),
                         g() % 2 ? 8 : 0, plain);
    }
    // pinned edge cases
    for (uint64_t wgs : wgss)
        for (double bias : {0.0, 0.1})
            for (int split = 0; split < 3; ++split) {
                check_layout({0}, 64, wgs, bias, split, 0, true);                               // n = 0
                check_layout(std::vector<IndexType>(3001, 0), 64, wgs, bias, split, 0, false);  // nnz = 0
                check_layout({0, 0}, 64, wgs, bias, split, 0, true);                            // n = 1
                check_layout({0, 9}, 64, wgs, bias, split, 0, true);
                std::vector<uint32_t> one(3000, 0);  // all entries in one row
                one[1234] = 70000;
                check_layout(row_ptr_of(one), 64, wgs, bias, split, 8, false);
                // a trailing and a middle run of empty rows longer than rmax: subdivided, and
                // (check_panels) no panel above rmax rows
                std::vector<uint32_t> trail(3000, 0), mid(3000, 3);
                std::fill(trail.begin(), trail.begin() + 1000, 3u);
                std::fill(mid.begin() + 1000, mid.begin() + 2500, 0u);
                check_layout(row_ptr_of(trail), 64, wgs, bias, split, 0, false);
                check_layout(row_ptr_of(mid), 64, wgs, bias, split, 0, false);
            }
    {
        // a bias on panels already at the row cap: the cut falls back to the even one
        const std::vector<IndexType> rp = row_ptr_of(std::vector<uint32_t>(64 * 64, 5));
        panel_options o;
        o.wgs = 64;
        o.P_first = min_panels(64 * 64, 64);
        panel_cut even, biased;
        CHECK(plan_panels("sweep", rp.data(), 64 * 64, rp.back(), 64, o, even) == 0);
        o.xbias = 0.1;
        CHECK(plan_panels("sweep", rp.data(), 64 * 64, rp.back(), 64, o, biased) == 0);
        CHECK(even.prow.size() == 65 && biased.prow == even.prow && biased.xbias == 0.0 && !biased.split_mode);
    }
    {
        // one row of 2^32 - 1 entries pads past 32 bits: rc 2
        const std::vector<IndexType> rp = {0, 0xFFFFFFFFu};
        panel_options o;
        o.allow_split = true;
        panel_cut c;
        sweep_units u;
        CHECK(plan_panels("build_sweep", rp.data(), 1, rp[1], 64, o, c) == 0);
        CHECK(plan_sweep_units("build_sweep", rp.data(), c.prow, c.split_mode, o.wgs, 0, 0.0, u) == 2);
        CHECK(!std::strcmp(get_error(), "build_sweep: padded entry count exceeds 32 bits"));
    }
    // binned: windows and segments
    for (int it = 0; it < 3000; ++it) {
        const uint64_t ncols = it < 64 ? uint64_t(it) : it % 3 ? g() % 200000 : g() % 60000000;
        const double bb[] = {0.0, 0.05, -0.05, 0.2, -0.24, 0.3};
        check_windows(ncols, wgss[g() % 3], bb[g() % 6]);
    }
    for (int it = 0; it < 300; ++it) {
        const uint64_t nwin = 1 + g() % 400, P = 1 + g() % 40, cus = wgss[g() % 3];
        std::vector<uint32_t> cnt(nwin * P), esc(nwin * P, 0);
        const int mode = it % 4;  // 0: nothing at all; 3: whole windows empty
        const uint64_t hole = g() % nwin;
        for (uint64_t k = 0; k < nwin * P; ++k) {
            cnt[k] = mode == 0 || (mode == 3 && (k / P) % 3 == hole % 3) ? 0 : g() % 4 ? uint32_t(g() % 300) : 0;
            if (mode == 2 && g() % 60 == 0)
                cnt[k] = uint32_t(g() % 200000);  // a heavy window
            esc[k] = mode >= 2 && cnt[k] ? uint32_t(g() % 3) : 0;
        }
        check_bin_units(cnt, esc, nwin, P, cus);
    }
    std::printf("OK layout\n");
    return 0;
}

// ---- the tile planner (layout.cpp plan_tiles) against a per-entry recomputation ----

static void check_tiles(const std::vector<uint32_t> &len)
{
    const std::vector<IndexType> rp = row_ptr_of(len);
    const IndexType n = IndexType(len.size());
    const uint64_t nnz = rp[n];
    // entry by entry: the compact index (among the non-empty rows) of the row that holds it
    std::vector<uint32_t> owner(nnz), ids;
    for (IndexType r = 0; r < n; ++r) {
        for (uint64_t k = rp[r]; k < rp[r + 1]; ++k)
            owner[k] = uint32_t(ids.size());
        if (len[r])
            ids.push_back(r);
    }
    for (int has_empty = 0; has_empty < 2; ++has_empty) {
        if (!has_empty && ids.size() < n)
            continue;  // (the build passes has_empty = some row is empty; with none, both forms)
        tile_plan t;
        set_error("");
        CHECK(plan_tiles(rp.data(), n, nnz, has_empty != 0, t) == 0 && !std::strlen(get_error()));
        CHECK(t.nnz_pad == (nnz + 511) / 512 * 512 && t.ntiles == t.nnz_pad / 512);
        CHECK(t.rowend.size() == t.nnz_pad / 32 && t.tile_info.size() == t.ntiles + 1);
        // bitmap bits: exactly the row ends (none in the padding)
        for (uint64_t k = 0; k < t.nnz_pad; ++k) {
            const bool end = k < nnz && (k + 1 == nnz || owner[k + 1] != owner[k]);
            CHECK(((t.rowend[k >> 5] >> (k & 31)) & 1u) == (end ? 1u : 0u));
        }
        // tile_info[t]: non-empty rows ended before entry 512 t, and whether that entry continues a row
        for (uint64_t i = 0; i <= t.ntiles; ++i) {
            const uint64_t k = 512 * i;
            const uint32_t ended = k == 0 ? 0 : k >= nnz ? uint32_t(ids.size()) : owner[k - 1] + (owner[k] != owner[k - 1]);
            const bool cont = k > 0 && k < nnz && owner[k] == owner[k - 1];
            CHECK(t.tile_info[i] == ((ended << 1) | (cont ? 1u : 0u)));
        }
        // row_id: the non-empty rows in order (only kept when some row is empty)
        CHECK(t.row_id == (has_empty ? ids : std::vector<uint32_t>()));
        // crossings: every non-empty row whose first and last entries lie in different tiles, in row order
        std::vector<uint32_t> want;
        for (uint32_t c = 0; c < ids.size(); ++c) {
            const uint64_t first = rp[ids[c]] / 512, last = (uint64_t(rp[ids[c] + 1]) - 1) / 512;
            if (last > first) {
                want.push_back(c);
                want.push_back(uint32_t(first));
                want.push_back(uint32_t(last));
            }
        }
        CHECK(t.cross == want);
    }
}

static int cmd_tiles()
{
    check_tiles({});           // no rows
    check_tiles({0, 0, 0});    // nnz = 0
    check_tiles({1});          // nnz = 1
    check_tiles({0, 1, 0});
    check_tiles({512});        // exactly one tile, in one row
    check_tiles({513});
    check_tiles({200, 312});   // nnz = 512 ending on a tile edge
    check_tiles({200, 312, 1});  // nnz = 513
    check_tiles({100, 1500, 7});  // one row over two tile boundaries, its crossing ending in a later tile
    check_tiles({1500});
    check_tiles({500, 12, 3});     // a row ending exactly on entry 511
    check_tiles({512, 512, 512});  // every row a whole tile: no crossing
    check_tiles({0, 0, 5, 0, 0, 600, 0, 3, 0, 0});  // leading, interior and trailing empty rows
    {
        std::vector<uint32_t> last(300, 0);  // all rows empty but the last
        last.back() = 1100;
        check_tiles(last);
    }
    std::mt19937_64 g(23);
    for (int it = 0; it < 300; ++it) {
        std::vector<uint32_t> len(g() % 400);
        const bool holes = it % 3 != 0;
        for (auto &l : len)
            l = g() % 50 == 0 ? 600 + uint32_t(g() % 601) : uint32_t(g() % 41) + (holes ? 0 : 1);
        check_tiles(len);
    }
    std::printf("OK tiles\n");
    return 0;
}

static int cmd_schedule()
{
    std::mt19937_64 g(9);
    for (int it = 0; it < 400; ++it) {
        const int nr = 1 + int(g() % 8);
        const uint32_t n = it % 17 == 0 ? 0 : uint32_t(g() % 3000);
        std::vector<IndexType> b(nr + 1, 0);
        for (int r = 1; r < nr; ++r)
            b[r] = (IndexType)(g() % (size_t(n) + 1));
        b[nr] = n;
        std::sort(b.begin(), b.end());
        for (int ex = SPMV_MGPU_GATHER; ex <= SPMV_MGPU_ALLGATHER; ++ex) {
            std::vector<int> cover(n, 0);
            std::vector<std::vector<spmv_xop>> all(nr);
            for (int r = 0; r < nr; ++r) {
                const int cnt = spmv_mgpu_schedule(ex, r, nr, b.data(), nullptr, 0);
                CHECK(cnt >= 0 && cnt <= 2 + 2 * nr);
                all[r].resize(cnt + 1);
                CHECK(spmv_mgpu_schedule(ex, r, nr, b.data(), all[r].data(), cnt) == cnt);
                all[r].resize(cnt);
                for (const spmv_xop &o : all[r]) {
                    CHECK(o.count > 0);
                    const uint64_t len = o.buf == SPMV_XBUF_SLICE ? b[r + 1] - b[r] : n;
                    CHECK(uint64_t(o.offset) + o.count <= len);
                    if (ex == SPMV_MGPU_GATHER && r == 0)
                        for (uint32_t i = o.offset; i < o.offset + o.count; ++i)
                            ++cover[i];
                }
            }
            if (ex == SPMV_MGPU_GATHER)
                for (uint32_t i = 0; i < n; ++i)
                    CHECK(cover[i] == 1);
            if (ex == SPMV_MGPU_ALLGATHER)  // every rank lists the same broadcasts
                for (int r = 1; r < nr; ++r) {
                    std::vector<spmv_xop> a, c;
                    for (const spmv_xop &o : all[0])
                        if (o.kind == SPMV_XOP_BCAST)
                            a.push_back(o);
                    for (const spmv_xop &o : all[r])
                        if (o.kind == SPMV_XOP_BCAST)
                            c.push_back(o);
                    CHECK(a.size() == c.size());
                    for (size_t k = 0; k < a.size(); ++k)
                        CHECK(std::memcmp(&a[k], &c[k], sizeof(spmv_xop)) == 0);
                }
        }
    }
    spmv_xop o;
    CHECK(spmv_mgpu_schedule(5, 0, 1, nullptr, &o, 1) == -1);
    std::printf("OK schedule\n");
    return 0;
}

// a part "lands" when its flag is set (release) by a producer thread: the stand-in for the DMA
// copy and its event; the wait spins with acquire, as hipEventSynchronize orders the host reads
struct Landing {
    std::atomic<int> done{0};
};

static int wait_flag(void *ready, std::string *err)
{
    Landing *l = static_cast<Landing *>(ready);
    for (int spin = 0; !l->done.load(std::memory_order_acquire); ++spin) {
        if (spin > 200000000) {
            *err = "part never landed";
            return 1;
        }
        std::this_thread::yield();
    }
    return 0;
}

static int cmd_accumulate()
{
    std::mt19937_64 g(3);
    for (int round = 0; round < 12; ++round) {
        const size_t units = 1 + round % 4, pieces = 1 + g() % 9;
        const uint64_t rows = round % 3 == 0 ? 1000 : 300000 + g() % 100000;  // below / above 2^18
        std::vector<ValueType> y(rows * units), want(rows * units);
        for (size_t i = 0; i < y.size(); ++i)
            y[i] = want[i] = ValueType(int(g() % 100)) / 4;
        std::vector<std::vector<ValueType>> stage(units, std::vector<ValueType>(rows));
        std::vector<ValueType> src(rows * units);
        for (size_t i = 0; i < src.size(); ++i) {
            src[i] = ValueType(int(g() % 100)) / 8;
            want[i] += src[i];
        }
        std::vector<Landing> land(units * pieces);
        std::vector<add_part> parts;
        for (size_t j = 0; j < pieces; ++j)  // landing order: piece j of every unit
            for (size_t u = 0; u < units; ++u) {
                const uint64_t b = rows * j / pieces, e = rows * (j + 1) / pieces;
                parts.push_back({y.data() + u * rows + b, stage[u].data() + b, e - b, &land[u * pieces + j]});
            }
        // one producer per unit copies its pieces into the staging buffer, in order
        std::vector<std::thread> prod;
        for (size_t u = 0; u < units; ++u)
            prod.emplace_back([&, u] {
                for (size_t j = 0; j < pieces; ++j) {
                    const uint64_t b = rows * j / pieces, e = rows * (j + 1) / pieces;
                    std::memcpy(stage[u].data() + b, src.data() + u * rows + b, (e - b) * sizeof(ValueType));
                    land[u * pieces + j].done.store(1, std::memory_order_release);
                    std::this_thread::sleep_for(std::chrono::microseconds(50 * (j % 3)));
                }
            });
        accum_options o;
        o.split = round % 2 == 0;
        o.prefault = round % 4 != 1;
        o.threads = 16;
        bool failed = true;
        std::string err;
        const double t = host_accumulate(parts.data(), parts.size(), wait_flag, o, &failed, &err);
        for (auto &p : prod)
            p.join();
        CHECK(!failed && t > 0);
        for (size_t i = 0; i < y.size(); ++i)
            CHECK(y[i] == want[i]);
    }
    // nothing to add: returns at once
    bool failed = true;
    accum_options o;
    host_accumulate(nullptr, 0, wait_flag, o, &failed, nullptr);
    CHECK(!failed);
    std::printf("OK accumulate\n");
    return 0;
}

static int cmd_verify()
{
    std::vector<ValueType> a(100), b(100);
    for (int i = 0; i < 100; ++i)
        a[i] = b[i] = ValueType(i) / 7;
    CHECK(verification(100, a.data(), b.data(), 0) == 0);
    b[17] += ValueType(1e-3);
    b[42] = std::nan("");
    CHECK(verification(100, a.data(), b.data(), 1) == 1);
    CHECK(verification(0, nullptr, nullptr, 0) == 0);
    IndexType ci[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, vl[2] = {0xFFFFFFFFu, 1};
    csr_hw_matrix m;
    std::memset(&m, 0, sizeof(m));
    m.nr_ci = ci;
    m.nr_val = vl;
    m.blocks = 2;
    const double mb = (double)storage_overhead(&m);
    const double want = (2.0 * 5 * 32 + (3.0 * 4294967295.0 + 1.0) * 128) / (8.0 * 1024 * 1024);
    CHECK(std::fabs(mb - want) <= want * 1e-6);
    CHECK(storage_overhead(nullptr) == 0);
    std::printf("OK verify\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "read"))
        return cmd_read(argv[2], argv[3]);
    if (argc >= 2 && !std::strcmp(argv[1], "partition"))
        return cmd_partition();
    if (argc >= 2 && !std::strcmp(argv[1], "slice"))
        return cmd_slice();
    if (argc >= 2 && !std::strcmp(argv[1], "layout"))
        return cmd_layout();
    if (argc >= 2 && !std::strcmp(argv[1], "tiles"))
        return cmd_tiles();
    if (argc >= 2 && !std::strcmp(argv[1], "schedule"))
        return cmd_schedule();
    if (argc >= 2 && !std::strcmp(argv[1], "accumulate"))
        return cmd_accumulate();
    if (argc >= 2 && !std::strcmp(argv[1], "verify"))
        return cmd_verify();
    std::fprintf(stderr, "usage: host_check read <mtx> <out> | partition | slice | layout | tiles | schedule | accumulate | verify\n");
    return 2;
}
