// sw_plan.cpp — the host driver's scan-planning policies (SURVEY.md §8 row
// a2; the reference packs one fixed 32-lane block order per launch,
// SWSolver.cu:309-359): which subjects go to the wavefront kernel, which
// blocks run by wave pairs, quads, 3-wave groups or tail pairs, and the
// longest-first work table of the merged launch (sw_scan_lpt) with its
// duration estimates.  Plain host code over a read-only view of a database
// (PlanDb); sw_db.cpp owns the databases, sw_capi.cpp caches the tables and
// uploads them.  scan_plan (at the end) puts the policies together: the form one
// scan takes, as a pure function of the database view, the query length,
// the scoring and the two adaptive routes.
#include "sw_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

namespace swplan {

namespace {
int32_t round_up(int64_t v, int64_t m) { return static_cast<int32_t>((v + m - 1) / m * m); }
}  // namespace

// Subjects longer than this go to the wavefront kernel.  A 64-lane block of
// the inter kernel takes time proportional to its longest subject, so very
// long subjects would become the kernel's critical path; measured on the C2
// workload (mean length 360): 1536 beats 3072 by 1.3x and 1024 by 1.03x
// (profiles/r01_tune_inter.jsonl); with the cooperative kernel for wide
// blocks the best is ~2048 (profiles/r01_tune_coop.jsonl).  Default: 5.7 x
// mean length, clamped.

//
// Small databases: the inter kernels put one 64-subject block on a wave and
// need ~2 waves per SIMD (2048 blocks, ~131k subjects) to fill the chip.
// Below ~1000 blocks the one-wave-per-subject wavefront kernel is the faster
// path for subjects of a few hundred residues and up (config C5, 10,000
// subjects of ~2000 aa vs a 5000-aa query: 2.7 TCUPS all-intra vs 0.62 TCUPS
// inter, profiles/r01_c5/), so everything longer than 64 residues goes there.
constexpr int64_t kSmallDbSubjects = 64 * 1000;

// Databases smaller than ~kFillSubjects (C2's 570,000 subjects are ~4.3
// 64-subject blocks per wave slot of the 256-CU GPU) — e.g. a rank's share
// of a strong-scaled database — have too few blocks to hide the widest ones:
// the scan time becomes the widest block's latency (width x passes / 2 for
// a wave pair) while a long subject on the wavefront kernel takes only
// (length + 64) steps.  The threshold then shrinks as (n / kFillSubjects)^0.4,
// measured on C2's 1/2, 1/4 and 1/8 shares with the merged longest-first
// launch (profiles/r02_strong/: 1/8 best near 900; two concurrent launches
// preferred 1,536-2,048 / 1,024 / 600-704).
constexpr double kFillSubjects = 570000.0;

int32_t default_long_threshold(const PlanDb& db) {
    if (db.n == 0) return 1536;
    const double mean = static_cast<double>(db.residues) / static_cast<double>(db.n);
    if (db.n < kSmallDbSubjects && mean >= 256) return 64;
    const double fill = db.n < kSmallDbSubjects ? 1.0 : std::min(1.0, static_cast<double>(db.n) / kFillSubjects);
    const double t = 5.7 * mean * std::pow(fill, 0.4);
    return static_cast<int32_t>(std::min(8192.0, std::max(fill < 1.0 ? 512.0 : 1024.0, t)));
}

// Leading (widest) blocks handled by the cooperative kernel: blocks whose
// one-wave time is a large share of the whole scan.  One wave of a W-column
// block costs ~W*qpad*3.5 VALU instructions at ~8.4 cycles each (2 waves per
// SIMD); the scan costs ~16 cycles per 64 cells over 1024 SIMDs.  Measured on
// C2 (2.05e8 residues, profiles/r01_tune_coop.jsonl): width 384 with long
// threshold 2048 is best, i.e. W ~ sum(residues) / 530000.  sw_opts
// coop_width overrides (tuning); 0 disables.
int32_t coop_blocks(const PlanDb& db, int divisor) {
    // divisor from the inter kernel's shape (swk::inter_coop_divisor): the
    // two-subjects-per-lane kernel wants a wider cut-off than int32 (measured
    // on C2: 1024 beats 386 and 640, profiles/r01_x2/); 0 = no coop kernel
    const int32_t forced = db.opts->coop_width;
    if (divisor <= 0 && forced < 0) return 0;
    int64_t wmin = divisor > 0 ? std::max<int64_t>(128, db.residues / divisor) : 0;
    if (forced >= 0) wmin = forced;
    if (wmin <= 0) return 0;
    int32_t n = 0;
    while (n < static_cast<int32_t>(db.nblocks) &&
           static_cast<int64_t>(db.blk_groups[n]) * swk::kGroupCols >= wmin)
        ++n;
    return n;
}

// Leading (widest) blocks of a two-strips scan handled by wave pairs
// (sw_inter_x2p): blocks at least `width` columns wide, width =
// residues / kPairDivisor (1024 on C2: with the biased cell 1,024 beat 256,
// 512 and none by 2-4 %, profiles/r01_tail2/; sw_opts pair_width
// overrides; 0 disables).
constexpr int64_t kPairDivisor = 200000;

// Waves per group for those blocks: pairs; sw_opts pair_group = 4 runs quads.
// Measured on C2's 1/8 share (profiles/r02_strong/): the inter kernel alone
// is fastest with quads over every block >= 64 wide (1.08 ms vs 1.29 for
// pairs), but beside the concurrent long-subject kernel, whose workgroups
// are dispatched first, a quad waits for a whole free workgroup slot and the
// scan is slower (2.21 vs 1.77 ms).
int pair_group(const PlanDb& db) { return db.opts->pair_group == 4 ? 4 : 2; }

int32_t pair_blocks(const PlanDb& db) {
    int64_t wmin = std::max<int64_t>(256, db.residues / kPairDivisor);
    if (db.opts->pair_width >= 0) wmin = db.opts->pair_width;
    if (wmin <= 0) return 0;
    int32_t n = 0;
    while (n < static_cast<int32_t>(db.nblocks) &&
           static_cast<int64_t>(db.blk_groups[n]) * swk::kGroupCols >= wmin)
        ++n;
    return n;
}

// ---- one merged launch, longest work first (sw_scan_lpt) -----------------
// Estimated duration of each workgroup of the merged grid: an inter tick (8
// columns x 64 rows of a 64-subject block, one wave) ~7.4 us and an intra
// step of sw_intra_x2<RI> ~0.157 us at RI = 6, scaled by its modeled
// SIMD cycles (RI x 28.8 + 80) — measured on C2's 1/8 share
// (profiles/r02_strong/traces/).  Only the order matters: the dispatcher
// starts workgroups in grid order, so the longest work starts first.
constexpr double kTickUs = 7.4;
// (0.157 us alone on a SIMD; inside the busy merged grid a step takes ~0.3
// us, profiles/r04_*/: with the doubled cost the long subjects start early
// enough, C2's 1/8 share +0.8 %)
double intra_step_us(int ri) { return 2 * 0.157 * (ri * 28.8 + 80.0) / (6 * 28.8 + 80.0); }
// Under linear gaps the intra step is relatively dearer than under affine
// ones (C2's 1/8 share, profiles/r05_trace/: intra / inter item medians 0.31
// against 0.28); scaling its estimates for linear scans by 85, 120 or 140 %
// made the share's reference-scoring rate 1.8, 0.8 and 3.6 % lower
// (profiles/r05_ab/lpt_lin_intra/): the same cost as under affine gaps.

// The widest group blocks of the merged launch run by quads: those at least
// kQuadFrac x the long threshold wide, whose pair latency would otherwise
// exceed the long subjects' (sw_opts quad_width w: at least w columns; 0: none)
// — on databases of fewer than kQuadMaxFill x kFillSubjects subjects only.
// Measured (profiles/r04_sweep_quads/): without quads C2 +1.0 %, its 1/2
// share +2.5 %, 1/4 +1.8 %, C3 unchanged, but the 1/8 share -19.6 % (its
// widest blocks' pair latency sets the span there).
constexpr double kQuadFrac = 0.67;
constexpr double kQuadMaxFill = 0.2;

int32_t lpt_quad_blocks(const PlanDb& db, int32_t npair) {
    int64_t wmin = static_cast<int64_t>(kQuadFrac * db.long_threshold);
    if (static_cast<double>(db.n) >= kQuadMaxFill * kFillSubjects) wmin = 0;
    if (db.opts->quad_width >= 0) wmin = db.opts->quad_width;
    if (wmin <= 0) return 0;
    int32_t n = 0;
    while (n < npair && static_cast<int64_t>(db.blk_groups[n]) * swk::kGroupCols >= wmin) ++n;
    return n;
}

// ... or, under affine gaps, by 3-wave groups (InterArgs::blk_tri): a query
// of P passes takes ceil(P / 3) rounds instead of ceil(P / 4), no wave idle
// in the last round, and the workgroup's fourth wave runs a single-wave
// block (the widest singles, beside the widest groups) — used where the
// rounds are as few as the quads' (P = 1, 2, 3, 5, 6, 9: a 375-aa query is 6
// passes of 64 rows), for the group blocks at least kTriFrac x the long
// threshold wide (sw_opts tri_width w: at least w columns; 0: none), on the
// databases that run quads.  Measured on C2's shares (profiles/r06_tri/):
// the 1/8 share's slowest rank 8,551 -> 9,001 GCUPS at 430 of its 891 (the
// widest pair blocks, the launch's critical path, take two rounds of a tri
// instead of three of a pair: -32 % latency at the same wave time, the
// spare wave doing work a single-wave workgroup would); 350-460 all +3 to +5
// %; the 1/4 share +0.7 % at 700 (-0.3 % at 530), the 1/2 share -0.4 % at
// 1,300 and worse below, C2 -1.3 % at 1,500 and worse below.
constexpr double kTriFrac = 0.48;

int32_t lpt_tri_blocks(const PlanDb& db, int32_t npair, int passes) {
    int64_t wmin = static_cast<double>(db.n) < kQuadMaxFill * kFillSubjects
                       ? static_cast<int64_t>(kTriFrac * db.long_threshold) : 0;
    if (db.opts->tri_width >= 0) wmin = db.opts->tri_width;
    if (wmin <= 0 || passes <= 0 || (passes + 2) / 3 > (passes + 3) / 4) return 0;
    int32_t n = 0;
    while (n < npair && static_cast<int64_t>(db.blk_groups[n]) * swk::kGroupCols >= wmin) ++n;
    return n;
}

// The narrowest blocks of the merged launch run by wave pairs (x2p_wg's tail
// range): the launch's last-dispatched work is its narrowest single-wave
// workgroups, which start together once the rest is placed, and the longest
// of them sets the end — C2's last 10 % ran at 73 % of the workgroup slots,
// 4 % of the launch idle (profiles/r05_trace/).  Pairs halve those blocks'
// latency for a few % more wave time on them.  Default: half a round of
// pair workgroups (2 blocks each; 2 workgroups per CU: as many blocks as
// workgroup slots) when the single-wave workgroups fill the GPU more than
// twice over, a quarter of that for more single-wave blocks than slots;
// sw_opts tail_pairs n: the narrowest n blocks.  C2 (256 CUs) over
// 128-3,072 blocks: 512 best, +1.5 % (1,024 +0.8 %, 3,072 -0.4 %); its 1/4
// share with 128: +0.6 % affine, +0.9 % linear, its 1/2 share +2.4 %
// linear; the 1/8 share (432 single-wave blocks: none) -0.6 % with 128
// (profiles/r05_ab/tail_pairs/).
int32_t lpt_tail_blocks(const PlanDb& db, int32_t npair, int passes) {
    const int64_t singles = db.nblocks - npair;
    if (passes < 2 || singles < 2) return 0;
    int64_t n = 0;
    if (db.opts->tail_pairs >= 0) {
        n = db.opts->tail_pairs;
    } else {
        const int64_t slots = 2 * static_cast<int64_t>(db.cus);  // workgroups per CU: 2
        if (slots > 0 && singles > 2 * swk::kWavesPerWG * slots) n = slots;
        else if (slots > 0 && singles > slots) n = slots / 4;  // (C2's 1/2 and 1/4 shares)
    }
    return static_cast<int32_t>(std::min<int64_t>(n, singles - 1));
}

// Ticks of a single-wave block (x2s_block: chained passes when ncols >= 32).
double single_ticks(int64_t ncols, int passes) {
    if (ncols <= 0) return 0;
    if (ncols >= 32 && passes > 1) return static_cast<double>(passes) * ncols / 8 + 1;
    return static_cast<double>(passes) * (ncols / 8 + 1);
}

double group_ticks_host(int64_t ncols, int passes, int G) {
    if (ncols <= 0 || passes <= 0) return 0;
    const int64_t S = ncols / 8 + 1;
    const int64_t per = std::max<int64_t>(S, 3 * G);
    int64_t t = 0;
    for (int p = std::max(0, passes - G); p < passes; ++p) t = std::max<int64_t>(t, (p / G) * per + 3 * (p % G) + S);
    return static_cast<double>(t);
}


LptPlan lpt_plan(const PlanDb& db, int32_t qpad, int rows, int32_t qpad_intra, int ri, int32_t npair, int32_t nquad,
                 int32_t ntail, bool affine, bool tri) {
    const int passes = qpad / rows;
    const double tick_us = kTickUs * rows / 64;  // a tick: 8 columns of one pass
    const int64_t nb = db.nblocks;
    const int64_t pwg = nquad + (npair - nquad + 1) / 2;
    // blocks [tail, nb) by pairs (x2p_wg's clamp: none unless tail lies in (npair, nb))
    const int64_t tail = ntail > 0 && nb - ntail > npair && nb - ntail < nb ? nb - ntail : nb;
    // tris: the spare wave of tri workgroup g runs single block npair + g
    const int64_t nspare = tri ? std::max<int64_t>(0, std::min<int64_t>(nquad, tail - npair)) : 0;
    const int64_t s0 = npair + nspare;  // the single-wave workgroups' first block
    const int64_t swg = (tail - s0 + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    const int64_t twg = (nb - tail + 1) / 2;
    const int64_t npairs = (db.nlong + 1) / 2;
    const int64_t iwg = (npairs + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    const int nch = qpad_intra / (swk::kLanes * ri);
    const double step_us = intra_step_us(ri);
    std::vector<std::pair<double, int32_t>> w;
    w.reserve(static_cast<size_t>(pwg + swg + twg + iwg));
    auto width = [&](int64_t b) { return static_cast<int64_t>(db.blk_groups[b]) * swk::kGroupCols; };
    for (int64_t g = 0; g < nquad; ++g) {
        double c = group_ticks_host(width(g), passes, tri ? 3 : 4);
        if (g < nspare) c = std::max(c, single_ticks(width(npair + g), passes));
        w.emplace_back(c * tick_us, g);
    }
    for (int64_t g = nquad; g < pwg; ++g) {
        double c = 0;
        for (int q = 0; q < 2; ++q) {
            const int64_t b = nquad + (g - nquad) * 2 + q;
            if (b < npair) c = std::max(c, group_ticks_host(width(b), passes, 2));
        }
        w.emplace_back(c * tick_us, static_cast<int32_t>(g));
    }
    for (int64_t g = 0; g < swg; ++g)  // widest first: the workgroup's first block bounds it
        w.emplace_back(single_ticks(width(s0 + g * swk::kWavesPerWG), passes) * tick_us,
                       static_cast<int32_t>(pwg + g));
    for (int64_t g = 0; g < twg; ++g) {  // tail pairs: the first block of two is the wider
        w.emplace_back(group_ticks_host(width(tail + 2 * g), passes, 2) * tick_us,
                       static_cast<int32_t>(pwg + swg + g));
    }
    // The longest pairs whose one-wave latency would exceed every inter
    // item's run in the pipelined form (a 128-row query chunk per wave,
    // ix2::intra_x2_wg PIPE; at most 4 chunks): a pair of one outlier subject
    // otherwise sets the launch's span alone (C2's 1/8 share: the 7,429-aa
    // subject's workgroup 1,275 us, every other one <= 1,224 us; pipelined,
    // 7,662 -> 8,082 GCUPS on one box, profiles/r04_*/).  They start first.
    // SW_LPT_PIPE=n forces n pairs (tests).
    const int nchp = (qpad_intra + 127) / 128;
    double inter_max = 0;
    for (const auto& e : w) inter_max = std::max(inter_max, e.first);
    // (in double: steps x chunks leaves int from a 2^30-residue subject's second chunk on)
    auto steps_us = [&](int64_t k) { return (static_cast<double>(db.llen[static_cast<size_t>(k)]) + swk::kLanes - 1) *
                                            nch * step_us; };
    auto pair_us = [&](int64_t p) { return steps_us(2 * p); };
    int64_t npipe = 0;
    if (nchp <= swk::kWavesPerWG) {
        if (db.opts->lpt_pipe >= 0) npipe = db.opts->lpt_pipe;
        else
            while (npipe < std::min<int64_t>(npairs, 4) && pair_us(npipe) > inter_max) ++npipe;
    }
    npipe = std::min(npipe, npairs);
    // The SHORTEST pairs in the pipelined form too (sw_opts lpt_pipe_tail n:
    // the last n pairs): the table ends with them, when the grid's slots
    // empty, and the pipeline cuts their latency to (length + 63 + 128
    // (chunks - 1)) steps of 2 rows per lane instead of (length + 63) of RI.
    // Default: 2 % of the pairs (to a multiple of 8) for linear scans of the
    // databases that run quads — measured on C2's 1/8 share under the
    // reference scoring (profiles/r06_tailpipe/): 12,794 / 12,802 / 12,803
    // -> 13,011 / 13,027 / 13,011 GCUPS with the last 32 of 1,561 pairs (16:
    // 13,018; 8, 24, 48, 64: 12,831, 12,879, 12,694, 12,772; 128 and more:
    // slower), affine scans within noise (their end is the tri groups').
    int64_t ntp = 0;
    if (db.opts->lpt_pipe_tail >= 0) ntp = db.opts->lpt_pipe_tail;
    else if (!affine && static_cast<double>(db.n) < kQuadMaxFill * kFillSubjects) ntp = (npairs * 2 / 100 + 4) / 8 * 8;
    if (nchp > swk::kWavesPerWG) ntp = 0;
    ntp = std::max<int64_t>(0, std::min(ntp, npairs - npipe));
    const int64_t pipe_tail = npairs - ntp;
    const int64_t npipe_wg = npipe / swk::kWavesPerWG;  // ordinary workgroups left with no pair
    for (int64_t g = npipe_wg; g < iwg; ++g) {
        const int64_t first = std::max<int64_t>(8 * g, 2 * npipe);  // its longest subject not pipelined
        if (first >= db.nlong || first >= 2 * pipe_tail) continue;
        w.emplace_back(steps_us(first), static_cast<int32_t>(-1 - g));
    }
    // (sw_scan_lpt item -1 - (iwg + pair)), ahead of everything
    for (int64_t p = 0; p < npipe; ++p) w.emplace_back(1e30 - p, static_cast<int32_t>(-1 - (iwg + p)));
    const double pstep_us = intra_step_us(2);
    for (int64_t p = pipe_tail; p < npairs; ++p)
        w.emplace_back((db.llen[static_cast<size_t>(2 * p)] + swk::kLanes - 1 + 128.0 * (nchp - 1)) * pstep_us,
                       static_cast<int32_t>(-1 - (iwg + p)));
    std::stable_sort(w.begin(), w.end(), [](const std::pair<double, int32_t>& x, const std::pair<double, int32_t>& y) {
        return x.first > y.first;
    });
    LptPlan out;
    out.order.resize(w.size());
    out.cost.resize(w.size());
    for (size_t k = 0; k < w.size(); ++k) {
        out.order[k] = w[k].second;
        out.cost[k] = static_cast<float>(w[k].first);
    }
    out.npipe = static_cast<int32_t>(npipe);
    out.pipe_tail = static_cast<int32_t>(pipe_tail);
    return out;
}

// ---- kernel shapes ---------------------------------------------------------
// Inter-kernel shape (sw_kernels.h InterShape); o.inter_variant "RxSG"
// overrides (tuning only).
swk::InterShape inter_shape(bool affine, int x2_ok, const sw_opts& o) {
    using swk::InterShape;
    // measured on MI355X (scripts/tune_inter.py, profiles/r01_tune_inter*.jsonl,
    // r01_x2s/): int16-safe scans (the common case) run the packed two-strips-
    // per-lane kernel sw_inter_x2s, one subject per lane, in its fp16 form
    // (biased cell, v_pk_maximum3_f16; C2 affine 9.4 TCUPS vs 6.25 int16),
    // always guarded (rescue chain fp16 -> int16 -> int32).  Otherwise int32:
    // affine 32x8, linear 64x8 (+ the cooperative kernel for wide blocks).
    // Beyond the static int16 bound the packed kernel runs guarded (blocks
    // reaching kSat16 are re-scored at int32); o.int16_guard = 0 disables that.
    // (Measured slower and removed in round 2: 16-bit-value and int32-profile
    // one-subject kernels, pair-table packing, two subjects per lane, the
    // column-skewed int32 kernel; their numbers are in profiles/r01_tune_*.)
    const bool y_ok = x2_ok == 2 || (x2_ok == 1 && o.int16_guard != 0);
    InterShape v = y_ok ? InterShape{64, 8, true, true} : InterShape{affine ? 32 : 64, 8};
    // o.inter_variant (tests / A-B only): "RxSG" int32 (32x8, 64x8),
    // "y32x8" the int16 two-strips kernel, "f32x8" / "f32x4" its fp16 form
    if (const char* e = o.inter_variant; e[0]) {
        int r = 0, g = 0;
        if (std::sscanf(e, "f%dx%d", &r, &g) == 2 && y_ok && r == 32 && (g == 8 || (g == 4 && affine)))
            v = InterShape{2 * r, g, true, true};
        else if (std::sscanf(e, "y%dx%d", &r, &g) == 2 && y_ok && r == 32 && g == 8)
            v = InterShape{2 * r, g, true, false};  // R = rows per pass
        else if (std::sscanf(e, "%dx%d", &r, &g) == 2 && g == 8 && (r == 32 || r == 64))
            v = InterShape{r, g};
    }
    return v;
}

std::string inter_kernel_name(const swk::InterShape& v, bool affine) {
    char b[96];
    if (v.x2s)
        std::snprintf(b, sizeof b, "sw_inter_x2s<%d,%d,%s%s>", v.R / 2, v.SG, affine ? "affine" : "linear",
                      v.f16 ? ",fp16" : "");
    else
        std::snprintf(b, sizeof b, "sw_inter<%d,%d,%s>", v.R, v.SG, affine ? "affine" : "linear");
    return b;
}

// int32 re-scoring of the blocks a 16-bit kernel put on the rescue list
// (launch_inter_rescue: sw_inter<32,8,affine> / <64,8,linear>).
int rescue_rows(bool affine) { return affine ? 32 : 64; }

// Rows per lane for the intra kernel: minimise
//   chunks * (steps per chunk) * (ops per step)
// with ops per step ~ RI * 3.7 (cells) + 8 (hand-off overhead); RI is even
// and at most 16 (register budget).
int intra_rows_for(int qlen, int longest) {
    int best_ri = 16;
    double best_cost = 1e300;
    for (int ri = 2; ri <= 16; ri += 2) {
        const int chunk = swk::kLanes * ri;
        const int nch = (qlen + chunk - 1) / chunk;
        const double cost = static_cast<double>(nch) * (longest + swk::kLanes - 1) * (ri * 3.7 + 8.0);
        if (cost < best_cost) { best_cost = cost; best_ri = ri; }
    }
    return best_ri;
}

int intra_x2_rows_for(int qlen, int longest, int wide, int forced) {
    // chunks x steps x (cell pairs per lane-step + conveyor/hand-off overhead)
    if (forced > 0) {  // sw_opts intra_x2_rows (tests: force a shape)
        const int ri = forced;
        if (ri == 4 || ri == 6 || ri == 8 || ri == 10 || ri == 12 || ri == 16) return ri;
        if (ri == swk::kIntraX2MaxRI && wide >= 1) return ri;
    }
    int best_ri = 16;
    double best_cost = 1e300;
    for (int ri : {4, 6, 8, 10, 12, 16, swk::kIntraX2MaxRI}) {
        if (ri == swk::kIntraX2MaxRI && wide < 2) continue;
        const int chunk = swk::kLanes * ri;
        const int nch = (qlen + chunk - 1) / chunk;
        // SIMD cycles per lane-step: ri rows x 6.8 ops x 4.25 + ~80 of conveyor
        const double cost = static_cast<double>(nch) * (longest + swk::kLanes - 1) * (ri * 28.8 + 80.0);
        if (cost < best_cost) {
            best_cost = cost;
            best_ri = ri;
        }
    }
    return best_ri;
}

// The rows per lane sw_scan_lpt is instantiated for: must agree with the
// switch at the end of launch_scan_lpt (sw_inter_x2.hip), which fails on
// any other.
bool lpt_supported(int ri) { return ri == 4 || ri == 6 || ri == 8; }

int32_t short_rows(int32_t qlen, int pass_rows) {
    const int32_t left = qlen - (round_up(qlen, pass_rows) / pass_rows - 1) * pass_rows;  // 1 .. pass_rows
    return (left + 1) / 2 <= pass_rows / 2 - 4 ? pass_rows / 2 - 4 : pass_rows / 2;
}

// ---- the form of a scan ----------------------------------------------------
PlanScoring plan_scoring(const int8_t* m, int go, int ge) {
    PlanScoring s;
    s.go = go;
    s.ge = ge;
    for (int k = 0; k < 625; ++k) {
        s.max_s = std::max<int>(s.max_s, m[k]);
        // The linear kernels keep S + gap in an int8 profile
        if (m[k] + go > 127) s.biased_fits = false;
    }
    return s;
}

PlanScoring plan_scoring_max(int max_entry, int go, int ge) {
    PlanScoring s;
    s.go = go;
    s.ge = ge;
    s.max_s = std::max(0, max_entry);
    s.biased_fits = max_entry + go <= 127;
    return s;
}

PlanScoring plan_scoring_pssm(const int8_t* rows, int32_t qlen, int go, int ge) {
    int mx = -128;
    for (int64_t k = 0; k < static_cast<int64_t>(qlen) * 25; ++k) mx = std::max<int>(mx, rows[k]);
    return plan_scoring_max(mx, go, ge);
}

// The biased cell's constants and the range of its patterns.  The guard is
// the fp16 cell's of earlier rounds, true scores of 4096 - 28 ge - 2 max S
// (which blocks are re-scored does not depend on the cell's format); the
// format would hold ~29,000.
//  * Highest: a lane below the guard has every H below it, H grows by at most
//    max S per cell, the diagonal sum adds one more entry, and a stored value
//    sits up to 26 ge above the true one (bias (15 + 7 + 2) ge, + 2 ge in the
//    profile): top = Z + sat_limit + 2 max S + 26 ge.
//  * Lowest: a floor is Z or above; below it go the rebased H, E and row -1
//    (8 ge), m = H - (go - ge), the row-group resets (16 ge), a row group's
//    first profile row (16 ge less) and the diagonal sum's entry, at most
//    once each: lowest = Z - go - 27 ge - 2 max |S|, the bound of the
//    admission rule 2 max S + 27 ge + go < 1024 with the matrix's negative
//    entries counted too.
// Z = 0x2000 leaves both ends thousands away from kCellMin and kCellMax for
// every admitted scheme over int8 entries.
// The affine cell does not rebase H: column 0's diagonal sum takes the 8 ge
// off through the hi0 image (hi - diff[1] mod 2^32, X2Lds in
// sw_inter_x2.hip), so the sum d is the rebased form's bit for bit and H
// keeps, across the sub-group boundary, the value it had just before the
// rebase: no pattern is read that the rebased form did not read, and the two
// bounds stand as they are.  diff[1], the dword 8 ge (2^16 + 1), is that
// constant, also for open below extend.
CellRange cell_range(int min_s, int max_s, int go, int ge) {
    CellRange c;
    c.z = 0x2000;
    const int ms = std::max(max_s, 1), abs_s = std::max({ms, -min_s, 0});
    // v in both halves as ONE 32-bit integer, v (2^16 + 1): adding or
    // subtracting it moves both halves by v, also for a negative v (go < ge),
    // whose dword is not two equal 16-bit patterns
    auto pair = [](int v) { return static_cast<uint32_t>(v) * 0x00010001u; };
    for (int j = 0; j < 32; ++j) c.step[j] = pair(j * ge + c.z);
    c.gog = pair(go - ge);
    c.diff[0] = pair(4 * ge);
    c.diff[1] = pair(8 * ge);
    c.diff[2] = pair(16 * ge);
    c.sat_limit = 4096 - 28 * ge - 2 * ms;
    c.lowest = c.z - go - 27 * ge - 2 * abs_s;
    c.guard = c.z + c.sat_limit;
    c.top = c.guard + 2 * ms + 26 * ge;
    return c;
}

ScanPlan scan_plan(const PlanDb& db, int32_t qlen, const PlanScoring& s, bool intra_i16_first, int32_t i16_span) {
    const sw_opts& O = *db.opts;
    const int max_s = s.max_s, go = s.go, ge = s.ge;
    ScanPlan p;
    // If S + gap does not fit the linear kernels' int8 profile, score with
    // the affine kernels (open == extend is the same DP).
    p.affine = go != ge || !s.biased_fits;
    const bool affine = p.affine;
    // The packed int16 kernel is exact when no H, E, F or H_diag + S can
    // leave int16: H <= qlen * max S, plus one profile entry (+ gap bias).
    // Beyond that bound the two-strips kernel runs guarded (saturating lanes
    // flag their block for int32 re-scoring) as long as one cell's increment
    // stays far inside the guard band (kSat16 leaves 1152).
    // Affine 16-bit scans run the fp16 biased cell first; its values sit up
    // to 26 ge above the true ones, so absurd gap / matrix scales (far beyond
    // any published scheme) go straight to int32.
    const bool f16_fits = 2 * max_s + 27 * ge + go < 1024;
    p.x2_ok = !f16_fits                                                   ? 0
              : (static_cast<int64_t>(qlen) + 2) * (max_s + go) < 32767 ? 2
              : (max_s + go < 1000 && ge < 1000)                       ? 1
                                                                       : 0;
    p.shape = inter_shape(affine, p.x2_ok, O);
    const int R = p.shape.R;
    // int32 re-scoring of blocks a 16-bit kernel flags near saturation
    p.rescue = swk::inter_needs_rescue(p.shape, p.x2_ok);
    p.f16 = p.shape.f16;
    p.qpad_rescue = p.rescue ? round_up(qlen, rescue_rows(affine)) : 0;
    // fp16 chain stage 2 (the int16 two-strips 32x8 kernel): 64-row passes
    // (the linear list kernel is the 48x4 shape: 96-row passes)
    const int list_rows = affine ? 64 : 96;
    p.qpad_list = p.f16 ? round_up(qlen, list_rows) : 0;

    // Long subjects: two per wave in packed fp16 (sw_intra_x2) when the guard
    // applies, with the int32 sw_intra re-scoring the subjects it flags
    // (sw_opts intra_x2 = 0: int32 only).
    p.intra_x2 = db.nlong && p.x2_ok >= 1 && O.intra_x2 != 0;
    p.intra_i16_first = intra_i16_first && p.intra_x2;
    // (20 rows per lane only where no merged launch can take the scan: no
    // inter blocks; where the fp16 bias of row 19 fits, as f16_fits; and by
    // the cost model for affine gaps only, see intra_x2_rows_for)
    const bool ri2_wide =
        db.nblocks == 0 && 2 * max_s + (swk::intra_bias_rows(swk::kIntraX2MaxRI) + 1) * ge + go < 1024;
    const int ri2_model =
        p.intra_x2 ? intra_x2_rows_for(qlen, db.long_max, ri2_wide ? (affine ? 2 : 1) : 0, O.intra_x2_rows) : 0;
    // Affine scans with inter blocks take the merged launch (intra rows 4, 6
    // or 8 only) even where the cost model prefers more rows per lane for the
    // long subjects alone: its tail pairs and looped grid win more (C3's long
    // queries at 8 rows: +1.3 %; under linear gaps the wider form stays,
    // -6.9 % at 8 rows: profiles/r05_ab/c3_ri8/).  A scan that does not take
    // the merged launch after all keeps the cost model's rows.
    const int ri2_lpt = (affine && ri2_model > 8 && db.nblocks && O.intra_x2_rows < 0) ? 8 : ri2_model;

    // two-strips scans: the widest blocks by wave pairs (at least two passes);
    // else the widest blocks first, one cooperative workgroup each (int32,
    // int8-profile paths)
    p.npair = (db.nblocks && swk::inter_has_pair(p.shape) && round_up(qlen, R) > R) ? pair_blocks(db) : 0;
    p.ncoop = (!p.npair && db.nblocks) ? coop_blocks(db, swk::inter_coop_divisor(p.shape)) : 0;
    p.qpad_coop = p.ncoop ? round_up(qlen, swk::kCoopRows) : 0;
    // the widest blocks the int16 kernel takes first (adapt_inter_i16_span)
    p.nr = (p.f16 && p.rescue && p.npair && !p.ncoop) ? i16_span : 0;

    // One merged launch for the fp16 scan, longest work first (sw_scan_lpt):
    // the inter groups + single waves and the long subjects' fp16 pass, when
    // the scan takes exactly that shape.  Measured (profiles/r02_strong/lpt/,
    // r02_round/): C2's 1/8 share 1.92 -> 1.45 ms, 1/4 2.57 -> 2.29.  On the
    // whole C2 database it was 2 % slower than two concurrent launches until
    // the launch drained its own rescue lists (no rescue launches or events
    // after it): now 7.19 -> 7.12 ms under affine scoring (C3 and C4's share
    // unchanged), but under linear gaps 4.57 -> 5.03 ms (profiles/r04_*/);
    // since round 5's tail pairs, looped grid and 96-row linear passes the
    // whole C2 database under linear gaps too: 16,512 -> 16,777 GCUPS
    // (profiles/r05_ab/lpt_linear_c2/).  Every scan of that shape takes it;
    // sw_opts lpt 0 / 1 forces either form.
    const bool lpt_want = O.lpt >= 0 ? O.lpt == 1 : true;
    p.lpt = lpt_want && db.nlong && db.nblocks && p.intra_x2 && !p.intra_i16_first && p.f16 && p.rescue &&
            p.npair && !p.ncoop && i16_span == 0 && lpt_supported(ri2_lpt);
    // The merged launch under linear gaps runs 96-row passes (48-row strips):
    // its widest blocks' wave groups need fewer rounds (a 375-aa query: 4
    // passes, one round of a quad, against 6 passes and two rounds of 64
    // rows), and the share's span is those blocks' latency;
    // the linear cell's registers leave room for the taller strips.  Affine
    // scans keep 64 rows (their E column would not fit).  sw_opts lpt_rows.
    p.lpt_rows = (p.lpt && !affine && O.lpt_rows != 64 && round_up(qlen, 96) > 96) ? 96 : 64;
    p.qpad_inter = round_up(qlen, p.lpt_rows == 96 ? 96 : R);
    p.re_last = p.shape.x2s ? short_rows(qlen, p.lpt_rows == 96 ? 96 : R) : 0;
    if (p.lpt) {
        const int passes = p.qpad_inter / p.lpt_rows;
        // (tri_width takes precedence: where tris apply, quad_width is not consulted)
        p.ntri = affine ? lpt_tri_blocks(db, p.npair, passes) : 0;
        p.nquad = p.ntri ? p.ntri : lpt_quad_blocks(db, p.npair);
        p.ntail = lpt_tail_blocks(db, p.npair, passes);
    }

    p.ri = db.nlong ? intra_rows_for(qlen, db.long_max) : 0;
    p.qpad_intra = p.ri ? round_up(qlen, static_cast<int64_t>(swk::kLanes) * p.ri) : 0;
    p.ri2 = p.lpt ? ri2_lpt : ri2_model;
    p.qpad_intra2 = p.ri2 ? round_up(qlen, static_cast<int64_t>(swk::kLanes) * p.ri2) : 0;
    p.multi_inter = p.qpad_inter > R || p.qpad_rescue > rescue_rows(affine) || p.qpad_coop > swk::kCoopRows ||
                    p.qpad_list > list_rows;
    p.multi_intra = (p.ri && p.qpad_intra > swk::kLanes * p.ri) || (p.ri2 && p.qpad_intra2 > swk::kLanes * p.ri2);

    if (db.nblocks) {
        p.kernel = inter_kernel_name(p.shape, affine);
        if (p.npair) p.kernel.replace(0, sizeof("sw_inter_x2s") - 1, "sw_inter_x2p");     // + wave pairs
        if (p.lpt_rows == 96) p.kernel.replace(p.kernel.find("<32,"), 4, "<48,");  // 48-row strips
        if (p.nr) p.kernel += "+int16[0," + std::to_string(p.nr) + ")";
        if (p.ntail) p.kernel += "+tail" + std::to_string(p.ntail);
        if (p.ntri) p.kernel += "+tri" + std::to_string(p.ntri);
        if (p.lpt) p.kernel += "+lpt";
    }
    p.intra_kernel = !db.nlong   ? "none"
                     : p.intra_x2 ? "sw_intra_x2<" + std::to_string(p.ri2) + (p.intra_i16_first ? ",int16>" : ">")
                                  : "sw_intra<" + std::to_string(p.ri) + (affine ? ",affine>" : ",linear>");
    return p;
}

void ScanPlan::set_drain(bool got_rows) {
    if (!lpt || !got_rows || drain) return;
    drain = true;
    ri = ri2;
    qpad_intra = qpad_intra2;  // the same rows per lane
    multi_intra = qpad_intra > swk::kLanes * ri;
    kernel += "+drain";
}

int64_t hits_scratch_bytes(int32_t qlen, int64_t slen) {
    if (qlen <= swk::kHitsChunkRows) return 0;
    return slen * swk::kHitsBndWords * static_cast<int64_t>(sizeof(int32_t));
}

std::vector<int64_t> hits_groups(int32_t qlen, const int64_t* slens, int64_t n, int64_t budget) {
    const std::vector<int32_t> qlens(static_cast<size_t>(std::max<int64_t>(n, 0)), qlen);
    return hits_groups(qlens.data(), slens, n, budget);
}

std::vector<int64_t> hits_groups(const int32_t* qlens, const int64_t* slens, int64_t n, int64_t budget) {
    std::vector<int64_t> ends;
    int64_t bytes = 0, k0 = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t b = hits_scratch_bytes(qlens[k], slens[k]);
        if (k > k0 && bytes + b > budget) {
            ends.push_back(k);
            k0 = k;
            bytes = 0;
        }
        bytes += b;
    }
    if (n > 0) ends.push_back(n);
    return ends;
}

int64_t align_dirs_bytes(int32_t qlen, int64_t slen) {
    return (qlen + slen + 1) * (static_cast<int64_t>(qlen) + 1);
}

std::vector<int64_t> align_groups(int32_t qlen, const int64_t* slens, int64_t n, int64_t budget) {
    std::vector<int64_t> ends;
    int64_t bytes = 0, k0 = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t b = align_dirs_bytes(qlen, slens[k]);
        if (k > k0 && bytes + b > budget) {
            ends.push_back(k);
            k0 = k;
            bytes = 0;
        }
        bytes += b;
    }
    if (n > 0) ends.push_back(n);
    return ends;
}

int32_t ranked_groups(int32_t nq, int64_t slots, int64_t score_bytes) {
    const int64_t budget = score_bytes == 0 ? kRankedRowsBudget : score_bytes;
    const int64_t rows = slots > 0 ? budget / (4 * slots) : nq;  // (no slots: rows cost nothing)
    return static_cast<int32_t>(std::max<int64_t>(1, std::min<int64_t>(nq, rows)));
}

int64_t hits_cost(int32_t qlen, int64_t slen) {
    if (qlen <= 0 || slen <= 0) return 0;
    constexpr int64_t kWaveRows = swk::kLanes * swk::kHitsRowsPerLane;
    const int64_t nblk = (slen + swk::kLanes - 1 + swk::kLanes - 1) / swk::kLanes;  // blocks of the slen + 63 steps
    int64_t rounds = 0;
    for (int64_t c0 = 0; c0 < qlen; c0 += swk::kHitsChunkRows) {
        const int64_t rows = std::min<int64_t>(qlen - c0, swk::kHitsChunkRows);
        rounds += nblk + 2 * ((rows + kWaveRows - 1) / kWaveRows - 1);
    }
    return rounds;
}

std::vector<int64_t> hits_order(const int32_t* qlens, const int64_t* slens, int64_t n) {
    std::vector<int64_t> order(static_cast<size_t>(std::max<int64_t>(n, 0))), cost(order.size());
    for (size_t k = 0; k < order.size(); ++k) {
        order[k] = static_cast<int64_t>(k);
        cost[k] = hits_cost(qlens[k], slens[k]);
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return cost[a] > cost[b]; });
    return order;
}

}  // namespace swplan
