// tests/native/pack_check.cpp — CPU check of the packed database layout
// (sw_pack.cpp) against the kernels' addressing of it, not the packer's own
// arithmetic: a short subject's column j is the byte at
//   blk_off[b] + (j / 16) * kGroupBytes + lane * kGroupCols + j % 16
// (sw_int32.h inter_block, sw_inter_x2.hip, sw_synth_fill_inter), a long
// subject's at loff[k] + j (the intra kernels, sw_synth_fill_intra), and a
// stored byte stands for the code kStored maps to it.  Every subject is in
// exactly one place with its residues, every other byte is the pad, the
// tables are the running sums and maxima of what the lanes hold, and the
// order is longest first and stable.  Built and run by tests/test_pack.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "sw_kernels.h"
#include "sw_pack.h"

static int failures = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++failures;                        \
        }                                      \
    } while (0)

static int64_t up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// longest first, file order within a length: a property of the order, not a
// second sort
static void check_order(const char* name, const std::vector<int64_t>& order, const std::vector<int64_t>& len) {
    const int64_t n = static_cast<int64_t>(len.size());
    CHECK(static_cast<int64_t>(order.size()) == n, "%s: order has %zu entries of %lld", name, order.size(),
          static_cast<long long>(n));
    if (static_cast<int64_t>(order.size()) != n) return;
    std::vector<int> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
        CHECK(order[i] >= 0 && order[i] < n && !seen[order[i]]++, "%s: order[%lld] is no permutation", name,
              static_cast<long long>(i));
        if (i == 0 || order[i] < 0 || order[i] >= n || order[i - 1] < 0 || order[i - 1] >= n) continue;
        const int64_t a = order[i - 1], b = order[i];
        CHECK(len[a] > len[b] || (len[a] == len[b] && a < b), "%s: order[%lld] not longest first and stable", name,
              static_cast<long long>(i));
    }
}

struct Case {
    std::string name;
    std::vector<int64_t> len;
    std::vector<int32_t> ids;  // empty: 0 .. n-1
    int32_t threshold;
};

static void check(const Case& c, bool all_codes = false) {
    const char* name = c.name.c_str();
    const int64_t n = static_cast<int64_t>(c.len.size());
    std::vector<int64_t> offs(n + 1, 0);
    for (int64_t k = 0; k < n; ++k) offs[k + 1] = offs[k] + c.len[k];
    std::vector<int32_t> ids(c.ids);
    if (ids.empty())
        for (int64_t k = 0; k < n; ++k) ids.push_back(static_cast<int32_t>(k));
    std::vector<uint8_t> res(static_cast<size_t>(offs[n]) + 1);
    bool used[25] = {};
    for (int64_t k = 0; k < n; ++k)
        for (int64_t j = 0; j < c.len[k]; ++j) used[res[offs[k] + j] = static_cast<uint8_t>((5 * k + 3 * j + 1) % 25)] = true;
    if (all_codes)
        for (int code = 0; code < 25; ++code) CHECK(used[code], "%s: the case does not use code %d", name, code);
    // the inverse of kStored, from kStored alone (and the kernels' copy of it)
    int code_of[26];
    for (int code = 0; code < 26; ++code) code_of[swk::kStored[code]] = code;
    for (int b = 0; b < 26; ++b) CHECK(swk::kCodeOf[b] == code_of[b], "kCodeOf[%d] is not kStored's inverse", b);
    std::map<int32_t, int64_t> subject_of;
    for (int64_t k = 0; k < n; ++k) subject_of[ids[k]] = k;

    swpack::Subjects subj;
    subj.n = n;
    subj.offsets = offs.data();
    subj.ids = ids.data();
    subj.residues = res.data();
    for (int want = 0; want < 2; ++want) {
        const swpack::Shape sh = swpack::plan(subj, c.threshold, want != 0);
        check_order(name, sh.order, c.len);
        if (failures) return;
        // the split: `>` the threshold is long
        int64_t nlong = 0, long_max = 0;
        for (int64_t k = 0; k < n; ++k)
            if (c.len[k] > c.threshold) ++nlong, long_max = std::max(long_max, c.len[k]);
        CHECK(sh.nlong == nlong && sh.long_max == long_max, "%s: nlong %lld (want %lld) long_max %d (want %lld)", name,
              static_cast<long long>(sh.nlong), static_cast<long long>(nlong), sh.long_max,
              static_cast<long long>(long_max));
        const int64_t nblocks = (n - nlong + swk::kLanes - 1) / swk::kLanes;
        CHECK(sh.nblocks == nblocks, "%s: %lld blocks, want %lld", name, static_cast<long long>(sh.nblocks),
              static_cast<long long>(nblocks));
        CHECK(static_cast<int64_t>(sh.loff.size()) == nlong + 1 && static_cast<int64_t>(sh.llen.size()) == nlong &&
                  static_cast<int64_t>(sh.lid.size()) == nlong,
              "%s: long table sizes", name);
        CHECK(static_cast<int64_t>(sh.blk_off.size()) == nblocks + 1 &&
                  static_cast<int64_t>(sh.blk_groups.size()) == nblocks &&
                  static_cast<int64_t>(sh.blk_cols.size()) == nblocks &&
                  static_cast<int64_t>(sh.blk_res.size()) == nblocks &&
                  static_cast<int64_t>(sh.lane_ids.size()) == nblocks * swk::kLanes &&
                  static_cast<int64_t>(sh.lane_len.size()) == (want ? nblocks * swk::kLanes : 0),
              "%s: block table sizes", name);
        if (failures) return;

        std::vector<int> placed(n, 0);
        // ---- long part
        std::vector<uint8_t> lbuf(static_cast<size_t>(sh.ltotal) + 1, 0xEE);
        for (int64_t k = 0; k < nlong; ++k) swpack::fill_long(subj, sh, k, lbuf.data() + sh.loff[k]);
        uint64_t at = 0;
        for (int64_t k = 0; k < nlong; ++k) {
            CHECK(sh.loff[k] == at && at % 64 == 0, "%s: loff[%lld]", name, static_cast<long long>(k));
            const auto it = subject_of.find(sh.lid[k]);
            CHECK(it != subject_of.end(), "%s: lid[%lld] = %d is no result id", name, static_cast<long long>(k), sh.lid[k]);
            if (it == subject_of.end()) return;
            const int64_t src = it->second, L = c.len[src];
            ++placed[src];
            CHECK(src == sh.order[k] && sh.llen[k] == L && L > c.threshold, "%s: long slot %lld", name,
                  static_cast<long long>(k));
            for (int64_t j = 0; j < up(L, 64); ++j) {
                const uint8_t byte = lbuf[sh.loff[k] + j];
                if (j < L)
                    CHECK(byte < 26 && code_of[byte] == res[offs[src] + j], "%s: long %lld column %lld", name,
                          static_cast<long long>(k), static_cast<long long>(j));
                else
                    CHECK(byte == swk::kPadCode, "%s: long %lld pad at %lld", name, static_cast<long long>(k),
                          static_cast<long long>(j));
            }
            at += static_cast<uint64_t>(up(L, 64));
        }
        CHECK(sh.loff[nlong] == at && sh.ltotal == at, "%s: ltotal", name);
        CHECK(lbuf[sh.ltotal] == 0xEE, "%s: fill_long wrote past the long part", name);

        // ---- inter part
        std::vector<uint8_t> buf(static_cast<size_t>(sh.total) + 1, 0xEE);
        for (int64_t b = 0; b < nblocks; ++b) swpack::fill_block(subj, sh, b, buf.data() + sh.blk_off[b]);
        at = 0;
        for (int64_t b = 0; b < nblocks; ++b) {
            CHECK(sh.blk_off[b] == at, "%s: blk_off[%lld]", name, static_cast<long long>(b));
            int64_t widest = 0, blk_res = 0;
            bool empty_seen = false;
            const int64_t cols = static_cast<int64_t>(sh.blk_groups[b]) * swk::kGroupCols;
            for (int lane = 0; lane < swk::kLanes; ++lane) {
                const int32_t id = sh.lane_ids[b * swk::kLanes + lane];
                int64_t L = 0, src = -1;
                if (id == -1) {
                    empty_seen = true;
                    CHECK(b == nblocks - 1, "%s: empty lane %d in block %lld, not the last", name, lane,
                          static_cast<long long>(b));
                } else {
                    CHECK(!empty_seen, "%s: block %lld lane %d follows an empty lane", name, static_cast<long long>(b),
                          lane);
                    const auto it = subject_of.find(id);
                    CHECK(it != subject_of.end(), "%s: lane id %d is no result id", name, id);
                    if (it == subject_of.end()) return;
                    src = it->second;
                    L = c.len[src];
                    ++placed[src];
                    CHECK(src == sh.order[nlong + b * swk::kLanes + lane] && L <= c.threshold,
                          "%s: block %lld lane %d holds subject %lld", name, static_cast<long long>(b), lane,
                          static_cast<long long>(src));
                }
                if (want) CHECK(sh.lane_len[b * swk::kLanes + lane] == L, "%s: lane_len", name);
                widest = std::max(widest, L);
                blk_res += L;
                CHECK(L <= cols, "%s: block %lld lane %d longer than the block", name, static_cast<long long>(b), lane);
                for (int64_t j = 0; j < cols; ++j) {
                    const uint8_t byte =
                        buf[sh.blk_off[b] + (j / 16) * swk::kGroupBytes + lane * swk::kGroupCols + j % 16];
                    if (j < L)
                        CHECK(byte < 26 && code_of[byte] == res[offs[src] + j], "%s: block %lld lane %d column %lld",
                              name, static_cast<long long>(b), lane, static_cast<long long>(j));
                    else
                        CHECK(byte == swk::kPadCode, "%s: block %lld lane %d pad at %lld", name,
                              static_cast<long long>(b), lane, static_cast<long long>(j));
                }
            }
            CHECK(sh.blk_groups[b] == (widest + 15) / 16, "%s: blk_groups[%lld] = %u, widest %lld", name,
                  static_cast<long long>(b), sh.blk_groups[b], static_cast<long long>(widest));
            CHECK(sh.blk_cols[b] == up(widest, 8) && sh.blk_cols[b] <= 16 * sh.blk_groups[b], "%s: blk_cols[%lld] = %u",
                  name, static_cast<long long>(b), sh.blk_cols[b]);
            CHECK(sh.blk_res[b] == blk_res, "%s: blk_res[%lld]", name, static_cast<long long>(b));
            at += static_cast<uint64_t>(sh.blk_groups[b]) * swk::kGroupBytes;
        }
        CHECK(sh.blk_off[nblocks] == at && sh.total == at, "%s: total", name);
        CHECK(buf[sh.total] == 0xEE, "%s: fill_block wrote past the inter part", name);
        for (int64_t k = 0; k < n; ++k)
            CHECK(placed[k] == 1, "%s: subject %lld placed %d times", name, static_cast<long long>(k), placed[k]);
        if (want)
            std::printf("%s: n %lld, %lld long (%llu bytes), %lld blocks (%llu bytes)\n", name,
                        static_cast<long long>(n), static_cast<long long>(sh.nlong),
                        static_cast<unsigned long long>(sh.ltotal), static_cast<long long>(sh.nblocks),
                        static_cast<unsigned long long>(sh.total));
    }
}

int main() {
    const int64_t edge[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40};
    // n subjects whose lengths walk the edges, in an order that is not sorted
    auto mixed = [&](int64_t n) {
        std::vector<int64_t> len(n);
        for (int64_t k = 0; k < n; ++k) len[k] = edge[(7 * k + 3) % 12];
        return len;
    };
    for (int64_t n : {0, 1, 63, 64, 65, 129}) {
        // threshold 9: 15 .. 40 long, 9 itself short
        check({"mixed-n" + std::to_string(n) + "-t9", mixed(n), {}, 9});
        check({"mixed-n" + std::to_string(n) + "-no-long", mixed(n), {}, 40});
        check({"mixed-n" + std::to_string(n) + "-all-long", std::vector<int64_t>(n, 17), {}, 16});
        check({"mixed-n" + std::to_string(n) + "-t0", mixed(n), {}, 0});  // only the empty subjects are short
    }
    check({"all-empty", std::vector<int64_t>(70, 0), {}, 5});  // two blocks of zero groups
    check({"one-at-threshold", {9, 10, 9}, {}, 9});
    {
        // many equal lengths, ids shuffled: file order within a length
        Case c{"equal-lengths-shuffled-ids", {}, {}, 8};
        for (int64_t k = 0; k < 129; ++k) {
            c.len.push_back(k % 3 == 0 ? 9 : 5);
            c.ids.push_back(static_cast<int32_t>((37 * k + 11) % 129));
        }
        check(c);
    }
    {
        Case c{"custom-ids", mixed(65), {}, 16};
        for (int64_t k = 0; k < 65; ++k) c.ids.push_back(static_cast<int32_t>(100000 - 1000 * k + (k % 2)));
        check(c);
    }
    check({"all-codes", mixed(65), {}, 32}, true);

    // length_order's std::stable_sort branch (a subject above 2^22 residues):
    // offsets only, planned and never filled; the order is the counting
    // sort's for the same lengths with that subject shortened
    {
        std::vector<int64_t> len = mixed(129);
        std::vector<int32_t> ids(129);
        for (int k = 0; k < 129; ++k) ids[k] = k;
        auto order_of = [&](int64_t longest) {
            len[77] = longest;
            std::vector<int64_t> offs(130, 0);
            for (int k = 0; k < 129; ++k) offs[k + 1] = offs[k] + len[k];
            swpack::Subjects subj;
            subj.n = 129;
            subj.offsets = offs.data();
            subj.ids = ids.data();
            const swpack::Shape sh = swpack::plan(subj, 16, false);
            check_order("stable-sort-branch", sh.order, len);
            CHECK(sh.nlong > 0 && sh.long_max == longest && sh.llen[0] == longest && sh.lid[0] == 77,
                  "stable-sort-branch: the longest subject leads the long part");
            return sh.order;
        };
        const std::vector<int64_t> big = order_of((int64_t(1) << 22) + 1), small = order_of(41);
        CHECK(big == small, "stable-sort-branch: the two sorts disagree");
        CHECK(swpack::length_order(nullptr, 0).empty(), "length_order of nothing");
        std::printf("stable-sort-branch: %zu subjects, same order\n", big.size());
    }
    if (failures) {
        std::printf("pack_check: %d failures\n", failures);
        return 1;
    }
    std::printf("pack_check ok\n");
    return 0;
}
