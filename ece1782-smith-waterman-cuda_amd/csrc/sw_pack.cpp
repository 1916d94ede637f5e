// sw_pack.cpp — the packed database layout (sw_pack.h): sort by length
// (descending, stable), route subjects longer than the threshold to the
// intra kernel, deal the rest into 64-lane blocks of 16-residue groups.
// Lanes past a subject's end hold kPadCode.
#include "sw_pack.h"

#include <algorithm>
#include <cstring>
#include <numeric>

#include "sw_kernels.h"
#include "sw_parallel.h"

namespace swpack {

namespace {

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// codes are stored as swk::kStored (the profile rows follow it)
void stored(uint8_t* d, const uint8_t* p, int64_t m) {
    for (int64_t j = 0; j < m; ++j) d[j] = swk::kStored[p[j]];
}

}  // namespace

std::vector<int64_t> length_order(const int64_t* offs, int64_t n) {
    std::vector<int64_t> order(n);
    int64_t maxl = 0;
    for (int64_t k = 0; k < n; ++k) maxl = std::max(maxl, offs[k + 1] - offs[k]);
    if (maxl > (int64_t(1) << 22)) {
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
            return offs[x + 1] - offs[x] > offs[y + 1] - offs[y];
        });
        return order;
    }
    std::vector<int64_t> start(static_cast<size_t>(maxl) + 2, 0);
    for (int64_t k = 0; k < n; ++k) ++start[static_cast<size_t>(maxl - (offs[k + 1] - offs[k]) + 1)];
    for (size_t l = 1; l < start.size(); ++l) start[l] += start[l - 1];
    for (int64_t k = 0; k < n; ++k) order[start[static_cast<size_t>(maxl - (offs[k + 1] - offs[k]))]++] = k;
    return order;
}

Shape plan(const Subjects& s, int32_t long_threshold, bool want_lane_len) {
    Shape sh;
    const int64_t n = s.n;
    sh.order = length_order(s.offsets, n);
    const std::vector<int64_t>& order = sh.order;
    int64_t nlong = 0;
    while (nlong < n && s.len(order[nlong]) > long_threshold) ++nlong;
    sh.nlong = nlong;
    sh.long_max = nlong ? static_cast<int32_t>(s.len(order[0])) : 0;

    // ---- intra (long) part: plain concatenation, 64-byte aligned starts
    sh.loff.resize(nlong + 1);
    sh.llen.resize(nlong);
    sh.lid.resize(nlong);
    uint64_t ltotal = 0;
    for (int64_t k = 0; k < nlong; ++k) {
        const int64_t src = order[k];
        sh.loff[k] = ltotal;
        sh.llen[k] = static_cast<int32_t>(s.len(src));
        sh.lid[k] = s.ids[src];
        ltotal += round_up(s.len(src), 64);
    }
    sh.loff[nlong] = ltotal;
    sh.ltotal = ltotal;

    // ---- inter part
    const int64_t nshort = n - nlong;
    const int64_t nblocks = (nshort + swk::kLanes - 1) / swk::kLanes;
    sh.nblocks = nblocks;
    sh.blk_off.resize(nblocks + 1);
    sh.blk_groups.resize(nblocks);
    sh.blk_cols.resize(nblocks);
    sh.lane_ids.assign(nblocks * swk::kLanes, -1);
    sh.blk_res.assign(nblocks, 0);
    uint64_t total = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int64_t first = nlong + b * swk::kLanes;  // longest subject of the block
        const int64_t w = round_up(s.len(order[first]), swk::kGroupCols);
        sh.blk_off[b] = total;
        sh.blk_groups[b] = static_cast<uint32_t>(w / swk::kGroupCols);
        sh.blk_cols[b] = static_cast<uint32_t>(round_up(s.len(order[first]), 8));
        total += static_cast<uint64_t>(sh.blk_groups[b]) * swk::kGroupBytes;
    }
    sh.blk_off[nblocks] = total;
    sh.total = total;
    sh.lane_len.assign(want_lane_len ? nblocks * swk::kLanes : 0, 0);
    swk::parallel_for(nblocks, [&](int64_t b) {
        for (int l = 0; l < swk::kLanes; ++l) {
            const int64_t k = nlong + b * swk::kLanes + l;
            if (k >= n) break;
            const int64_t src = order[k];
            sh.lane_ids[b * swk::kLanes + l] = s.ids[src];
            sh.blk_res[b] += s.len(src);
            if (want_lane_len) sh.lane_len[b * swk::kLanes + l] = static_cast<int32_t>(s.len(src));
        }
    });
    return sh;
}

Location locate(int64_t p, int64_t nlong) {
    if (p < nlong) return {p, -1};
    return {(p - nlong) / swk::kLanes, static_cast<int32_t>((p - nlong) % swk::kLanes)};
}

// one block's bytes: [group][lane][16 codes], kPadCode past each subject
void fill_block(const Subjects& s, const Shape& sh, int64_t b, uint8_t* dst) {
    std::memset(dst, swk::kPadCode, static_cast<size_t>(sh.blk_groups[b]) * swk::kGroupBytes);
    for (int l = 0; l < swk::kLanes; ++l) {
        const int64_t k = sh.nlong + b * swk::kLanes + l;
        if (k >= s.n) break;
        const int64_t src = sh.order[k], L = s.len(src);
        const uint8_t* p = s.residues + s.offsets[src];
        uint8_t* d = dst + l * swk::kGroupCols;
        int64_t j = 0;
        for (; j + swk::kGroupCols <= L; j += swk::kGroupCols, d += swk::kGroupBytes) stored(d, p + j, swk::kGroupCols);
        if (j < L) stored(d, p + j, L - j);
    }
}

void fill_long(const Subjects& s, const Shape& sh, int64_t k, uint8_t* dst) {
    const int64_t src = sh.order[k];
    std::memset(dst, swk::kPadCode, sh.loff[k + 1] - sh.loff[k]);
    stored(dst, s.residues + s.offsets[src], s.len(src));
}

void Shape::release_upload_tables() {
    order = {};
    loff = {};
    lid = {};
    blk_off = {};
    blk_cols = {};
    lane_ids = {};
    lane_len = {};
}

}  // namespace swpack
