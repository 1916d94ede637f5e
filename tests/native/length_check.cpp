// tests/native/length_check.cpp — the host units at length, on the CPU:
// planning (sw_plan.cpp), packing (sw_pack.cpp) and calibration
// (sw_calib.cpp) for subjects and queries past 2^15 and 2^16, for one subject
// of 2^30 residues (the longest sw_db_create accepts) and for queries of
// 65,544 and 2^24 rows.  Built by tests/test_length_plan.py with
// -fsanitize=undefined,signed-integer-overflow -fno-sanitize-recover, so an
// int that overflows on the way to a count ends the program; what the
// sanitiser cannot see (a count that is merely wrong) is compared with a
// recount in 64 or 128 bits.  Never runs on a GPU, never loaded into Python.
//
//   length_check LENGTHS   LENGTHS: a text file, the subjects' lengths in
//                          database order (tests/length_support.py's G)
//
// Planning: the database view of G in three layouts (everything in lanes,
// everything long, the library's own split) and of G beside a 2^30-residue
// subject (offsets only), under BLOSUM62 11/1 and BLOSUM50 linear 2, with the
// library's own policies and with the merged launch forced: scan_plan's
// conditions (plan_check.cpp's), the merged launch's work table decoded as the
// kernel decodes it (every block and every long pair once), hits_groups /
// align_groups (every hit in exactly one group, sizes recounted),
// hits_cost / hits_order, intra_rows_for / intra_x2_rows_for.  The kernel
// names are printed; tests/test_gpu_lengths.py asserts the same names on the
// device.  Packing: pack_check.cpp's read-back through the kernels'
// addressing for G in the lane and the long layout.  Calibration: length_bin
// and the rank table's entries at 70,001, 2^30 and INT32_MAX.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sw_calib.h"
#include "sw_kernels.h"
#include "sw_pack.h"
#include "sw_plan.h"

static int failures = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++failures;                        \
        }                                      \
    } while (0)

using i128 = __int128;

static int64_t up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

static sw_opts policy_defaults() {
    sw_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = static_cast<int32_t>(sizeof o);
    for (int32_t* f : {&o.lpt_pipe, &o.quad_width, &o.pair_width, &o.pair_group, &o.coop_width, &o.tail_pairs,
                       &o.tri_width, &o.lpt_pipe_tail, &o.lpt, &o.lpt_rows, &o.intra_x2, &o.intra_x2_rows,
                       &o.int16_guard})
        *f = -1;
    return o;
}

// A database of these lengths, offsets only, and its view under a threshold
// (0: the library's own, as sw_db_create chooses it).
struct Db {
    std::vector<int64_t> len, offs;
    std::vector<int32_t> ids;
    swpack::Subjects subj;
    swpack::Shape sh;
    sw_opts o;
    swplan::PlanDb v;
    Db(const std::vector<int64_t>& lengths, int32_t threshold, const sw_opts& opts) : len(lengths), o(opts) {
        const int64_t n = static_cast<int64_t>(len.size());
        offs.assign(n + 1, 0);
        for (int64_t k = 0; k < n; ++k) offs[k + 1] = offs[k] + len[k];
        for (int64_t k = 0; k < n; ++k) ids.push_back(static_cast<int32_t>(k));
        subj.n = n;
        subj.offsets = offs.data();
        subj.ids = ids.data();
        v.n = n;
        v.residues = offs[n];
        v.opts = &o;
        v.cus = 256;
        if (threshold == 0) threshold = swplan::default_long_threshold(v);
        sh = swpack::plan(subj, threshold, false);
        v.nblocks = sh.nblocks;
        v.nlong = sh.nlong;
        v.long_threshold = threshold;
        v.long_max = sh.long_max;
        v.blk_groups = sh.blk_groups.data();
        v.llen = sh.llen.data();
    }
    Db(const Db&) = delete;
};

// The layout's tables against a 64-bit recount from the lengths alone.
static void check_shape(const char* name, const Db& d) {
    std::vector<int64_t> sorted(d.len);
    std::stable_sort(sorted.begin(), sorted.end(), [](int64_t a, int64_t b) { return a > b; });
    int64_t nlong = 0;
    for (int64_t L : sorted) nlong += L > d.v.long_threshold;
    CHECK(d.sh.nlong == nlong && d.sh.long_max == (nlong ? sorted[0] : 0), "%s: nlong %lld long_max %d", name,
          (long long)d.sh.nlong, d.sh.long_max);
    uint64_t at = 0;
    for (int64_t k = 0; k < nlong && k < d.sh.nlong; ++k) {
        CHECK(d.sh.loff[k] == at && d.sh.llen[k] == sorted[k] && d.sh.llen[k] > 0, "%s: long slot %lld", name, (long long)k);
        at += static_cast<uint64_t>(up(sorted[k], 64));
    }
    CHECK(d.sh.ltotal == at && d.sh.loff.back() == at, "%s: ltotal %llu, recount %llu", name,
          (unsigned long long)d.sh.ltotal, (unsigned long long)at);
    const int64_t nshort = static_cast<int64_t>(sorted.size()) - nlong;
    const int64_t nblocks = (nshort + swk::kLanes - 1) / swk::kLanes;
    CHECK(d.sh.nblocks == nblocks, "%s: %lld blocks, recount %lld", name, (long long)d.sh.nblocks, (long long)nblocks);
    at = 0;
    for (int64_t b = 0; b < nblocks && b < d.sh.nblocks; ++b) {
        const int64_t widest = sorted[nlong + b * swk::kLanes];
        int64_t res = 0;
        for (int64_t k = nlong + b * swk::kLanes; k < std::min<int64_t>(nlong + (b + 1) * swk::kLanes, sorted.size()); ++k)
            res += sorted[k];
        CHECK(d.sh.blk_off[b] == at && d.sh.blk_groups[b] == static_cast<uint64_t>((widest + 15) / 16) &&
                  d.sh.blk_cols[b] == static_cast<uint64_t>(up(widest, 8)) && d.sh.blk_res[b] == res,
              "%s: block %lld: off %llu groups %u cols %u res %lld (widest %lld)", name, (long long)b,
              (unsigned long long)d.sh.blk_off[b], d.sh.blk_groups[b], d.sh.blk_cols[b], (long long)d.sh.blk_res[b],
              (long long)widest);
        at += static_cast<uint64_t>((widest + 15) / 16) * swk::kGroupBytes;
    }
    CHECK(d.sh.total == at, "%s: total %llu, recount %llu", name, (unsigned long long)d.sh.total, (unsigned long long)at);
}

// The merged launch's table against the kernel's decoding (plan_check.cpp's scenario()).
static void check_lpt(const char* name, const Db& d, const swplan::ScanPlan& p) {
    const swplan::PlanDb& db = d.v;
    const bool tri = p.ntri > 0;
    const swplan::LptPlan t = swplan::lpt_plan(db, p.qpad_inter, p.lpt_rows, p.qpad_intra2, p.ri2, p.npair, p.nquad,
                                               p.ntail, p.affine, tri);
    const int64_t nb = db.nblocks, npair = p.npair, nquad = p.nquad, ntail = p.ntail;
    const int64_t pwg = nquad + (npair - nquad + 1) / 2;
    const int64_t tail = ntail > 0 && nb - ntail > npair && nb - ntail < nb ? nb - ntail : nb;
    const int64_t nspare = tri ? std::max<int64_t>(0, std::min<int64_t>(nquad, tail - npair)) : 0;
    const int64_t s0 = npair + nspare;
    const int64_t twg = pwg + (tail - s0 + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    const int64_t npairs = (db.nlong + 1) / 2;
    const int64_t niwg = (npairs + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    std::vector<int> blk_seen(nb, 0), pair_seen(npairs, 0);
    for (size_t k = 0; k < t.order.size(); ++k) {
        const int32_t it = t.order[k];
        if (k) CHECK(t.cost[k] <= t.cost[k - 1], "%s: entry %zu out of order", name, k);
        CHECK(t.cost[k] >= 0 && std::isfinite(t.cost[k]), "%s: entry %zu costs %g", name, k, t.cost[k]);
        if (it >= 0) {
            const int64_t wgi = it;
            if (wgi >= pwg && wgi < twg) {
                for (int w = 0; w < swk::kWavesPerWG; ++w) {
                    const int64_t b = s0 + (wgi - pwg) * swk::kWavesPerWG + w;
                    if (b < tail) ++blk_seen[b];
                }
            } else if (wgi >= twg) {
                for (int q = 0; q < 2; ++q) {
                    const int64_t b = tail + (wgi - twg) * 2 + q;
                    if (b < nb) ++blk_seen[b];
                }
            } else if (wgi < nquad) {
                ++blk_seen[wgi];
                if (tri && npair + wgi < s0) ++blk_seen[npair + wgi];
            } else {
                for (int q = 0; q < 2; ++q) {
                    const int64_t b = nquad + (wgi - nquad) * 2 + q;
                    if (b < npair) ++blk_seen[b];
                }
            }
        } else {
            const int64_t g = -1 - static_cast<int64_t>(it);
            if (g < niwg) {
                for (int w = 0; w < swk::kWavesPerWG; ++w) {
                    const int64_t pr = g * swk::kWavesPerWG + w;
                    if (pr < npairs && pr >= t.npipe && pr < t.pipe_tail) ++pair_seen[pr];
                }
            } else {
                const int64_t pr = g - niwg;
                CHECK(pr >= 0 && pr < npairs && (pr < t.npipe || pr >= t.pipe_tail), "%s: pipelined pair %lld", name, (long long)pr);
                if (pr >= 0 && pr < npairs) ++pair_seen[pr];
            }
        }
    }
    for (int64_t b = 0; b < nb; ++b) CHECK(blk_seen[b] == 1, "%s: block %lld scanned %d times", name, (long long)b, blk_seen[b]);
    for (int64_t pr = 0; pr < npairs; ++pr) CHECK(pair_seen[pr] == 1, "%s: pair %lld scanned %d times", name, (long long)pr, pair_seen[pr]);
    // the first ordinary workgroup's estimate, recounted in double: steps x chunks x the step's cost
    const int64_t g0 = t.npipe / swk::kWavesPerWG, first = std::max<int64_t>(8 * g0, 2 * t.npipe);
    if (first < db.nlong && first < 2 * static_cast<int64_t>(t.pipe_tail)) {
        const double want = (static_cast<double>(db.llen[first]) + swk::kLanes - 1) *
                            (p.qpad_intra2 / (swk::kLanes * p.ri2)) * swplan::intra_step_us(p.ri2);
        double got = -1;
        for (size_t k = 0; k < t.order.size(); ++k)
            if (t.order[k] == static_cast<int32_t>(-1 - g0)) got = t.cost[k];
        CHECK(std::fabs(got - want) <= 1e-6 * want, "%s: the longest workgroup's estimate %g, recount %g", name, got, want);
    }
}

static void check_plan(const char* name, const Db& d, int32_t qlen, int max_s, int go, int ge) {
    swplan::PlanScoring s;
    s.max_s = max_s;
    s.go = go;
    s.ge = ge;
    s.biased_fits = max_s + go <= 127;
    swplan::ScanPlan p = swplan::scan_plan(d.v, qlen, s, false, 0);
    const int64_t heights[6][2] = {{p.qpad_inter, p.lpt_rows == 96 ? 96 : p.shape.R},
                                   {p.qpad_intra, 64 * p.ri},
                                   {p.qpad_intra2, 64 * p.ri2},
                                   {p.qpad_rescue, swplan::rescue_rows(p.affine)},
                                   {p.qpad_list, p.affine ? 64 : 96},
                                   {p.qpad_coop, swk::kCoopRows}};
    for (int k = 0; k < 6; ++k) {
        const int64_t q = heights[k][0], rows = heights[k][1];
        if (q == 0 && k != 0) continue;
        CHECK(rows > 0 && q > 0 && q == up(qlen, rows), "%s: padded length %d: %lld for %lld rows, qlen %d", name, k,
              (long long)q, (long long)rows, qlen);
    }
    CHECK((p.ri != 0) == (d.v.nlong != 0) && (p.ri2 != 0) == p.intra_x2, "%s: ri %d ri2 %d", name, p.ri, p.ri2);
    CHECK(p.npair >= 0 && p.npair <= d.v.nblocks && p.ncoop >= 0 && p.ncoop <= d.v.nblocks && p.nquad <= p.npair &&
              p.ntail >= 0 && p.ntail <= d.v.nblocks,
          "%s: block ranges %d %d %d %d", name, p.npair, p.ncoop, p.nquad, p.ntail);
    CHECK(p.kernel.empty() == (d.v.nblocks == 0) && (p.intra_kernel == "none") == (d.v.nlong == 0), "%s: names", name);
    if (d.v.nlong) {
        const int ri = swplan::intra_rows_for(qlen, d.v.long_max);
        CHECK(ri >= 2 && ri <= 16 && ri % 2 == 0 && ri == p.ri, "%s: intra_rows_for %d", name, ri);
        for (int wide = 0; wide < 3; ++wide) {
            const int r2 = swplan::intra_x2_rows_for(qlen, d.v.long_max, wide, -1);
            CHECK(r2 == 4 || r2 == 6 || r2 == 8 || r2 == 10 || r2 == 12 || r2 == 16 || (r2 == 20 && wide == 2),
                  "%s: intra_x2_rows_for %d (wide %d)", name, r2, wide);
        }
    }
    if (p.lpt) {
        check_lpt(name, d, p);
        p.set_drain(true);
        CHECK(p.ri == p.ri2 && p.qpad_intra == p.qpad_intra2, "%s: drain", name);
    }
    std::printf("%s: %s | %s ri %d ri2 %d\n", name, p.kernel.c_str(), p.intra_kernel.c_str(), p.ri, p.ri2);
}

// hits_groups / align_groups / hits_cost / hits_order over every subject as one call's hits.
static void check_groups(const char* name, const Db& d, int32_t qlen) {
    const int64_t n = static_cast<int64_t>(d.len.size());
    const int64_t* slens = d.len.data();
    for (int which = 0; which < 2; ++which) {
        const std::vector<int64_t> ends = which ? swplan::align_groups(qlen, slens, n) : swplan::hits_groups(qlen, slens, n);
        const int64_t budget = which ? swplan::kAlignDirsBudget : swplan::kHitsScratchBudget;
        CHECK(!ends.empty() && ends.back() == n, "%s: groups %d end at %lld of %lld", name, which,
              ends.empty() ? -1LL : (long long)ends.back(), (long long)n);
        int64_t k0 = 0;
        for (size_t g = 0; g < ends.size(); ++g) {
            CHECK(ends[g] > k0, "%s: group %zu of %d is empty", name, g, which);
            i128 bytes = 0;
            for (int64_t k = k0; k < ends[g]; ++k) {
                const i128 want = which ? (static_cast<i128>(qlen) + slens[k] + 1) * (static_cast<i128>(qlen) + 1)
                                        : (qlen > swk::kHitsChunkRows ? static_cast<i128>(slens[k]) * swk::kHitsBndWords * 4 : 0);
                const int64_t got = which ? swplan::align_dirs_bytes(qlen, slens[k]) : swplan::hits_scratch_bytes(qlen, slens[k]);
                CHECK(got == want && (got > 0 || (!which && qlen <= swk::kHitsChunkRows)), "%s: bytes of hit %lld (%d): %lld", name,
                      (long long)k, which, (long long)got);
                bytes += want;
            }
            // a group fits the budget unless it is one hit; the next hit would not have fitted
            CHECK(bytes <= budget || ends[g] - k0 == 1, "%s: group %zu of %d over the budget", name, g, which);
            if (ends[g] < n) {
                const i128 next = which ? static_cast<i128>(swplan::align_dirs_bytes(qlen, slens[ends[g]]))
                                        : static_cast<i128>(swplan::hits_scratch_bytes(qlen, slens[ends[g]]));
                CHECK(bytes + next > budget, "%s: group %zu of %d closed early", name, g, which);
            }
            k0 = ends[g];
        }
        std::printf("%s: %s groups %zu\n", name, which ? "align" : "hits", ends.size());
    }
    const std::vector<int32_t> qlens(static_cast<size_t>(n), qlen);
    const std::vector<int64_t> order = swplan::hits_order(qlens.data(), slens, n);
    std::vector<int> seen(n, 0);
    CHECK(static_cast<int64_t>(order.size()) == n, "%s: hits_order size", name);
    for (size_t k = 0; k < order.size(); ++k) {
        CHECK(order[k] >= 0 && order[k] < n && !seen[order[k]]++, "%s: hits_order is no permutation", name);
        const int64_t c = swplan::hits_cost(qlen, slens[order[k]]);
        // the recount: per chunk, ceil((slen + 63) / 64) blocks and two rounds per further wave
        const int64_t wave = swk::kLanes * swk::kHitsRowsPerLane;
        i128 want = 0;
        for (int64_t c0 = 0; c0 < qlen; c0 += swk::kHitsChunkRows)
            want += (static_cast<i128>(slens[order[k]]) + 63 + 63) / 64 +
                    2 * ((std::min<int64_t>(qlen - c0, swk::kHitsChunkRows) + wave - 1) / wave - 1);
        CHECK(c > 0 && c == want, "%s: hits_cost %lld", name, (long long)c);
        if (k) CHECK(c <= swplan::hits_cost(qlen, slens[order[k - 1]]), "%s: hits_order not by cost", name);
    }
}

// pack_check.cpp's read-back: every column of every subject through the kernels' addressing.
static void check_packing(const char* name, const std::vector<int64_t>& len, int32_t threshold) {
    const int64_t n = static_cast<int64_t>(len.size());
    std::vector<int64_t> offs(n + 1, 0);
    for (int64_t k = 0; k < n; ++k) offs[k + 1] = offs[k] + len[k];
    std::vector<int32_t> ids(n);
    for (int64_t k = 0; k < n; ++k) ids[k] = static_cast<int32_t>(3 * ((7 * k + 5) % n) + 1);
    std::vector<int64_t> subject_of(3 * n + 2, -1);
    for (int64_t k = 0; k < n; ++k) subject_of[ids[k]] = k;
    std::vector<uint8_t> res(static_cast<size_t>(offs[n]) + 1);
    // (a residue that depends on the column's high bits too: a column read mod 2^15 or 2^16 differs)
    auto code = [](int64_t k, int64_t j) { return static_cast<uint8_t>((5 * k + 3 * j + (j >> 15) * 7 + (j >> 16) * 11 + 1) % 25); };
    for (int64_t k = 0; k < n; ++k)
        for (int64_t j = 0; j < len[k]; ++j) res[offs[k] + j] = code(k, j);
    int code_of[26];
    for (int c = 0; c < 26; ++c) code_of[swk::kStored[c]] = c;
    swpack::Subjects subj;
    subj.n = n;
    subj.offsets = offs.data();
    subj.ids = ids.data();
    subj.residues = res.data();
    const swpack::Shape sh = swpack::plan(subj, threshold, true);
    std::vector<int> placed(n, 0);
    std::vector<uint8_t> lbuf(static_cast<size_t>(sh.ltotal) + 1, 0xEE);
    for (int64_t k = 0; k < sh.nlong; ++k) swpack::fill_long(subj, sh, k, lbuf.data() + sh.loff[k]);
    int64_t bad = 0;
    for (int64_t k = 0; k < sh.nlong; ++k) {
        const int64_t src = subject_of[sh.lid[k]], L = len[src];
        ++placed[src];
        CHECK(sh.llen[k] == L && L > threshold && sh.loff[k] % 64 == 0, "%s: long slot %lld", name, (long long)k);
        for (int64_t j = 0; j < up(L, 64); ++j) {
            const uint8_t byte = lbuf[sh.loff[k] + j];
            bad += j < L ? !(byte < 26 && code_of[byte] == code(src, j)) : byte != swk::kPadCode;
        }
    }
    CHECK(lbuf[sh.ltotal] == 0xEE, "%s: fill_long wrote past the long part", name);
    std::vector<uint8_t> buf(static_cast<size_t>(sh.total) + 1, 0xEE);
    for (int64_t b = 0; b < sh.nblocks; ++b) swpack::fill_block(subj, sh, b, buf.data() + sh.blk_off[b]);
    for (int64_t b = 0; b < sh.nblocks; ++b) {
        const int64_t cols = static_cast<int64_t>(sh.blk_groups[b]) * swk::kGroupCols;
        for (int lane = 0; lane < swk::kLanes; ++lane) {
            const int32_t id = sh.lane_ids[b * swk::kLanes + lane];
            const int64_t src = id < 0 ? -1 : subject_of[id], L = src < 0 ? 0 : len[src];
            if (src >= 0) ++placed[src];
            CHECK(sh.lane_len[b * swk::kLanes + lane] == L && L <= threshold && L <= cols, "%s: block %lld lane %d", name,
                  (long long)b, lane);
            for (int64_t j = 0; j < cols; ++j) {
                const uint8_t byte = buf[sh.blk_off[b] + (j / 16) * swk::kGroupBytes + lane * swk::kGroupCols + j % 16];
                bad += j < L ? !(byte < 26 && code_of[byte] == code(src, j)) : byte != swk::kPadCode;
            }
        }
    }
    CHECK(buf[sh.total] == 0xEE, "%s: fill_block wrote past the inter part", name);
    CHECK(bad == 0, "%s: %lld bytes differ from the subjects' residues or the pad", name, (long long)bad);
    for (int64_t k = 0; k < n; ++k) CHECK(placed[k] == 1, "%s: subject %lld placed %d times", name, (long long)k, placed[k]);
    std::printf("%s: n %lld, %lld long (%llu bytes), %lld blocks (%llu bytes)\n", name, (long long)n, (long long)sh.nlong,
                (unsigned long long)sh.ltotal, (long long)sh.nblocks, (unsigned long long)sh.total);
}

static void check_calibration() {
    // length_bin: four bins per octave, from the leading bit and the two below it
    const struct { uint32_t L; int bin; } bins[] = {{70001u, 4 * 16 + 0},       // 2^16 x 1.068
                                                     {1u << 30, 4 * 30},
                                                     {(1u << 30) - 1, 4 * 29 + 3},
                                                     {INT32_MAX, 4 * 30 + 3},
                                                     {65535u, 4 * 15 + 3},
                                                     {65536u, 4 * 16},
                                                     {32767u, 4 * 14 + 3},
                                                     {32768u, 4 * 15}};
    for (const auto& b : bins) {
        CHECK(swcalib::length_bin(b.L) == b.bin && b.bin < swcalib::kLBins, "length_bin(%u) = %d, want %d", b.L,
              swcalib::length_bin(b.L), b.bin);
        // the bin's range holds L: 2^e (1 + f / 4) <= L < 2^e (1 + (f + 1) / 4)
        const int e = b.bin >> 2, f = b.bin & 3;
        CHECK(std::ldexp(1.0 + f / 4.0, e) <= b.L && b.L < std::ldexp(1.0 + (f + 1) / 4.0, e), "length_bin(%u): range", b.L);
    }
    // the rank table of 70,002 entries; a subject of 2^30 or INT32_MAX residues reads its last one
    sw_calib c{};
    c.size = static_cast<int32_t>(sizeof c);
    c.qlen = 568;
    c.n_db = 64;
    c.n_fit = 64;
    c.a = 12.5;
    c.c = 7.25;
    c.sigma = 6.0;
    const int32_t max_len = 70001;
    std::vector<int32_t> adj(static_cast<size_t>(max_len) + 2, 0x5A5A5A5A);
    swcalib::rank_table(c, max_len, adj.data());
    CHECK(adj[0] == 0 && adj[max_len + 1] == 0x5A5A5A5A, "rank_table wrote %d entries too few or too many", max_len + 1);
    for (int32_t L : {1, 32767, 32768, 65535, 65536, 70001}) {
        const long long want = std::llround(4096.0L * 7.25L * std::log(static_cast<long double>(L)));
        CHECK(std::llabs(adj[L] - want) <= 1, "rank_table[%d] = %d, want %lld", L, adj[L], want);
    }
    for (int32_t L : {70001, 1 << 30, INT32_MAX}) {
        const int32_t a = adj[std::min(L, max_len)];
        const int64_t r = swcalib::rank_value(100, L, a);
        CHECK(r == 100 * swcalib::kRankScale - adj[max_len], "rank_value at %d", L);
        const int64_t key = swcalib::rank_key(r, INT32_MAX - 1);
        CHECK(swcalib::rank_key_id(key) == INT32_MAX - 1 && key > INT64_MIN, "rank_key at %d", L);
    }
    // a table of one entry and of none beyond adj[0]
    int32_t one[2] = {7, 7};
    swcalib::rank_table(c, 0, one);
    CHECK(one[0] == 0 && one[1] == 7, "rank_table(0)");
    std::printf("calibration: bins %d %d %d, adj[70001] %d\n", swcalib::length_bin(70001), swcalib::length_bin(1u << 30),
                swcalib::length_bin(INT32_MAX), adj[max_len]);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: length_check LENGTHS\n");
        return 2;
    }
    std::vector<int64_t> G;
    if (FILE* f = std::fopen(argv[1], "r")) {
        long long v;
        while (std::fscanf(f, "%lld", &v) == 1) G.push_back(v);
        std::fclose(f);
    }
    if (G.size() < 8) {
        std::printf("no lengths in %s\n", argv[1]);
        return 2;
    }
    const sw_opts o = policy_defaults();
    sw_opts merged = o;  // tests/test_gpu_lengths.py's merged profile
    merged.lpt = 1;
    merged.pair_width = 16;
    merged.intra_x2_rows = 8;
    std::vector<int64_t> huge(G);
    huge.insert(huge.begin() + 3, int64_t(1) << 30);
    const struct { const char* name; int max_s, go, ge; } scorings[] = {{"b62-11-1", 11, 11, 1}, {"b50-2-2", 15, 2, 2}};
    const struct { const char* name; const std::vector<int64_t>* len; int32_t threshold; const sw_opts* opts; } dbs[] = {
        {"lanes", &G, 100000, &o},      {"long", &G, 1, &o},           {"own", &G, 0, &o},
        {"split", &G, 3000, &o},        {"split-merged", &G, 3000, &merged},
        {"huge-long", &huge, 1, &o},    {"huge-own", &huge, 0, &o},    {"huge-split-merged", &huge, 3000, &merged},
        {"huge-lanes", &huge, 1 << 30, &o}};
    const int32_t qlens[] = {568, 900, 1300, 32760, 32776, 35213, 65544, 1 << 24};
    for (const auto& dbc : dbs) {
        const Db d(*dbc.len, dbc.threshold, *dbc.opts);
        check_shape(dbc.name, d);
        std::printf("%s: threshold %d, %lld long, %lld blocks, widest %u groups\n", dbc.name, d.v.long_threshold,
                    (long long)d.v.nlong, (long long)d.v.nblocks, d.v.nblocks ? d.sh.blk_groups[0] : 0u);
        for (int32_t qlen : qlens) {
            for (const auto& sc : scorings)
                check_plan((std::string(dbc.name) + "-" + sc.name + "-q" + std::to_string(qlen)).c_str(), d, qlen, sc.max_s,
                           sc.go, sc.ge);
            check_groups((std::string(dbc.name) + "-q" + std::to_string(qlen)).c_str(), d, qlen);
        }
    }
    check_packing("pack-lanes", G, 100000);
    check_packing("pack-long", G, 1);
    check_calibration();
    if (failures) {
        std::printf("length_check: %d failures\n", failures);
        return 1;
    }
    std::printf("length_check ok\n");
    return 0;
}
