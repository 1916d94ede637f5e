// sw_plan.h — the host driver's scan-planning policies (sw_plan.cpp): plain
// functions of a read-only database view, so the policies and the merged
// launch's work table can be built and checked without a GPU
// (tests/test_plan.py).  scan_plan() is where the form of a scan is decided:
// gap model, kernel shapes, rows per lane, block counts, merged launch or
// not, and the names sw_last_kernel reports; sw_capi.cpp's scan_impl_body
// only enqueues what the plan says.  sw_db.cpp owns the databases and the
// device copies of the tables.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "sw_amd.h"
#include "sw_kernels.h"

namespace swplan {

// What the policies read of a database (sw_db.cpp plan_view: the counts
// and tables of sw_db's swpack::Shape, sw_pack.h).
struct PlanDb {
    int64_t n = 0;                        // subjects
    int64_t residues = 0;
    int64_t nblocks = 0;                  // 64-subject inter blocks
    int64_t nlong = 0;                    // long subjects (the wavefront kernel's)
    int32_t long_threshold = 0;
    int32_t long_max = 0;                 // the longest long subject
    const uint32_t* blk_groups = nullptr;  // [nblocks] 16-column groups per block, widest first
    const int32_t* llen = nullptr;         // [nlong] long subjects' lengths, longest first
    const sw_opts* opts = nullptr;         // the handle's kernel-form overrides
    int cus = 0;                           // the device's compute units
};

// Subjects longer than this go to the wavefront kernel (n, residues only).
int32_t default_long_threshold(const PlanDb& db);
// Leading (widest) blocks of the cooperative int32 kernel (divisor from the
// inter kernel's shape; 0 = none).
int32_t coop_blocks(const PlanDb& db, int divisor);
// Waves per group of the separate pair launch (2 or 4).
int pair_group(const PlanDb& db);
// Leading (widest) blocks of a two-strips scan run by wave groups.
int32_t pair_blocks(const PlanDb& db);
// The merged launch's widest group blocks by quads, or under affine gaps by
// 3-wave groups (0: none), and its narrowest blocks by pairs.
int32_t lpt_quad_blocks(const PlanDb& db, int32_t npair);
int32_t lpt_tri_blocks(const PlanDb& db, int32_t npair, int passes);
int32_t lpt_tail_blocks(const PlanDb& db, int32_t npair, int passes);
// Duration model (SIMD-busy microseconds and ticks of 8 columns of a pass).
double intra_step_us(int ri);
double single_ticks(int64_t ncols, int passes);
double group_ticks_host(int64_t ncols, int passes, int G);

// Shape of the inter kernel for this gap model (swk::InterShape; x2_ok as
// ScanPlan's); o.int16_guard / o.inter_variant override the choice (tests, A/B).
swk::InterShape inter_shape(bool affine, int x2_ok, const sw_opts& o);
// Name of the per-wave inter kernel launch_inter() runs, e.g. "sw_inter_x2s<32,8,affine,fp16>".
std::string inter_kernel_name(const swk::InterShape& v, bool affine);
// Query rows per strip of the int32 re-scoring of listed blocks (launch_inter_rescue).
int rescue_rows(bool affine);
// Query rows per lane the int32 intra kernel uses for this query (2..16, even).
int intra_rows_for(int qlen, int longest);
// ... and the two-subjects fp16 one.  wide: 0 = rows per lane 4..16; 1 = 20
// too when forced (sw_opts intra_x2_rows, > 0: a forced shape); 2 = 20 by the
// cost model too.  scan_plan allows 20 only where no merged launch can take
// the scan (no inter blocks) and the fp16 bias of row 19 fits, and picks it
// only for affine gaps (the linear cell lost 35 % at 20 on C5: its cheaper
// steps need the third wave per SIMD).
int intra_x2_rows_for(int qlen, int longest, int wide, int forced);
// Rows per lane the merged launch is built for.
bool lpt_supported(int ri);
// Rows per strip (Re) of the last pass of a two-strips scan with passes of
// pass_rows = 2 R query rows.  The kernels have two forms of a pass, R rows
// per strip and R - 4 (sw_inter_x2.hip x2s_pass's RL): R - 4 when two strips
// of that height hold the rows the query has left for its last pass, else R.
int32_t short_rows(int32_t qlen, int pass_rows);

// What a scan's form depends on of its scoring.
struct PlanScoring {
    int max_s = 0;            // the matrix's largest entry (at least 0)
    int go = 0, ge = 0;
    bool biased_fits = true;  // matrix + gap fits the linear kernels' int8 profile
};
PlanScoring plan_scoring(const int8_t* matrix625, int go, int ge);
// The same for a position-specific scoring matrix (sw_pssm): rows is
// [qlen][25] int8; max_s and biased_fits follow the table's entries, so a
// table that contains a matrix's largest entry plans as that matrix.
PlanScoring plan_scoring_pssm(const int8_t* rows, int32_t qlen, int go, int ge);
// ... and from the largest entry alone (what sw_pssm_create records).
PlanScoring plan_scoring_max(int max_entry, int go, int ge);

// The form of one scan (qlen > 0): everything sw_capi.cpp's enqueue stages
// read.  Final when scan_plan returns, but for set_drain.
struct ScanPlan {
    bool affine = false;    // the affine kernels (go != ge, or the biased profile does not fit)
    // 2 = provably int16-safe (any packed kernel may run); 1 = a guarded
    // packed kernel may run (saturating blocks re-scored at int32); 0 = int32 only
    int x2_ok = 0;
    swk::InterShape shape{};
    bool rescue = false;    // the inter kernel may flag blocks for re-scoring
    bool f16 = false;       // ... in its fp16 form (rescue chain fp16 -> int16 -> int32)
    bool intra_x2 = false;  // long subjects two per wave in fp16 first
    bool intra_i16_first = false;  // ... or in int16 first (the adaptive route, where intra_x2)
    int ri = 0;             // rows per lane: the int32 long-subject kernel
    int ri2 = 0;            // ... and the fp16 / int16 one
    // the query padded to each kernel's pass height (0: the kernel does not run)
    int32_t qpad_inter = 0, qpad_intra = 0, qpad_intra2 = 0, qpad_rescue = 0, qpad_list = 0, qpad_coop = 0;
    int32_t npair = 0;      // widest blocks by wave groups
    int32_t ncoop = 0;      // ... or by the cooperative int32 kernel
    int32_t nr = 0;         // widest blocks in int16 beside the fp16 launch (the span used)
    bool lpt = false;       // one merged launch (sw_scan_lpt)
    bool drain = false;     // ... that re-scores what it flags itself (set_drain)
    int lpt_rows = 64;      // its query rows per pass: 64, or 96 under linear gaps
    // the two-strips kernels' short last pass: rows per strip (short_rows of
    // the inter launch's pass height; 0: another kernel shape, every row runs)
    int32_t re_last = 0;
    int32_t ntri = 0, nquad = 0, ntail = 0;  // its 3-wave groups, quads (= ntri when tris run), tail pairs
    bool multi_inter = false, multi_intra = false;  // more than one pass: boundary rows needed
    // what sw_last_kernel / sw_last_intra_kernel report; kernel is empty
    // when no inter kernel runs (the handle keeps the last scan's name),
    // intra_kernel "none" without long subjects
    std::string kernel, intra_kernel;

    // The one runtime fact the plan cannot know: whether the merged launch
    // obtained boundary rows of its own (sw_db.cpp ensure_rbnd; lpt only).
    // With them it drains its rescue lists itself, the int32 long-subject
    // stage at the fp16 form's rows per lane: ri = ri2, qpad_intra (and
    // multi_intra, a function of the two) follow, the name gets "+drain".
    void set_drain(bool got_rows);
};

// The inter scan's biased "fp16" cell (sw_inter_x2.hip x2s_pass): each 16-bit
// half of a cell dword holds the unsigned integer true + bias + Z.  Sums and
// differences are 32-bit integer ops on the dword and the maxima are packed
// fp16 ops, so every value an addition or a maximum reads must be a positive
// normal fp16 pattern, [kCellMin, kCellMax]: there the unsigned order is the
// fp16 order, a maximum returns one of its inputs bit for bit whatever the
// kernel's denormal mode, and no carry or borrow crosses bit 16.
constexpr int kCellMin = 0x0400, kCellMax = 0x7BFF;
struct CellRange {
    int z = 0;               // the offset Z of every stored value
    uint32_t step[32] = {};  // InterArgs::f16_step: the pair (j ge + Z) in both halves, the floor of bias j ge
    uint32_t gog = 0;        // f16_gog: (go - ge) (2^16 + 1), the dword whose subtraction takes go - ge off both halves
    uint32_t diff[3] = {};   // f16_diff: the pairs (4 ge, 8 ge, 16 ge)
    int sat_limit = 0;       // a lane whose true maximum reaches this flags its block
    int lowest = 0;          // the lowest pattern an addition or a maximum can read
    int guard = 0;           // the guard's pattern at bias 0: Z + sat_limit
    int top = 0;             // the highest pattern of a lane below the guard: guard + 2 max S + the largest bias
};
// min_s, max_s: bounds of the scoring matrix's (or table's) entries.
CellRange cell_range(int min_s, int max_s, int go, int ge);

// intra_i16_first, i16_span: the adaptive routes (sw_capi.cpp
// adapt_intra_i16_first, adapt_inter_i16_span; span within 0 .. nblocks).
ScanPlan scan_plan(const PlanDb& db, int32_t qlen, const PlanScoring& s, bool intra_i16_first, int32_t i16_span);

// The merged launch's work table: entries longest (estimated) first.  An
// entry >= 0 is an inter workgroup of x2p_wg's numbering (groups, then
// single waves, then tail pairs); -1 - g an intra workgroup g (4 pairs) for
// g < iwg, or -1 - (iwg + p) pair p in the pipelined form (the longest
// npipe pairs and the pairs from pipe_tail on).
struct LptPlan {
    std::vector<int32_t> order;
    std::vector<float> cost;  // the estimate of each entry, microseconds
    int32_t npipe = 0;
    int32_t pipe_tail = 0;
};
LptPlan lpt_plan(const PlanDb& db, int32_t qpad, int rows, int32_t qpad_intra, int ri, int32_t npair, int32_t nquad,
                 int32_t ntail, bool affine, bool tri);

// The hit table's scratch (sw_hits.hip): a hit needs its chunk boundary row
// only, swk::kHitsBndWords int32 per subject column, and only when the query
// is longer than one chunk of swk::kHitsChunkRows rows; nothing grows with
// qlen x slen.
int64_t hits_scratch_bytes(int32_t qlen, int64_t slen);
constexpr int64_t kHitsScratchBudget = int64_t(1) << 30;
// Hits [ends[g - 1], ends[g]) (ends[-1] = 0) run as one launch: consecutive
// hits whose scratch fits the budget; a single hit over the budget forms its
// own group.  ends.back() == n; empty for n == 0.
std::vector<int64_t> hits_groups(int32_t qlen, const int64_t* slens, int64_t n, int64_t budget = kHitsScratchBudget);
// ... of hits with a query each (sw_hit_stats_batch: a launch mixes queries);
// a hit whose query fits one chunk adds 0 bytes.  Scratch belongs to the hit,
// never to the subject: two queries on one subject get a boundary row each.
std::vector<int64_t> hits_groups(const int32_t* qlens, const int64_t* slens, int64_t n,
                                 int64_t budget = kHitsScratchBudget);
// A hit's serial length in the kernel's own rounds (sw_hits.hip: a round is
// 64 steps of every wave between two barriers): per chunk, the blocks of its
// slen + 63 steps plus two rounds for each further wave that holds a query
// row.  0 for an empty query or subject (the workgroup returns at once).
int64_t hits_cost(int32_t qlen, int64_t slen);
// The order hits launch in: cost descending, equal costs in the caller's
// order, so the longest wavefronts start in the first wave of workgroups.
std::vector<int64_t> hits_order(const int32_t* qlens, const int64_t* slens, int64_t n);

// The traceback's direction array (sw_align.hip): one byte per cell, stored
// diagonal-major T[d][i], d in [0, qlen + slen], i in [0, qlen].
int64_t align_dirs_bytes(int32_t qlen, int64_t slen);
constexpr int64_t kAlignDirsBudget = int64_t(1) << 30;
// Hits [ends[g - 1], ends[g]) (ends[-1] = 0) of one sw_align call run as one
// launch: consecutive hits, in the caller's order, whose direction arrays fit
// the budget; a single hit over the budget forms its own group.
// ends.back() == n; empty for n == 0.
std::vector<int64_t> align_groups(int32_t qlen, const int64_t* slens, int64_t n, int64_t budget = kAlignDirsBudget);

// Score rows a batch ranked by E-value keeps (sw_scan_batch_hits_ranked: a
// query's fit precedes its ranking, so the queries of a group keep a row
// each): G = max(1, min(nq, score_bytes / (4 slots))), slots = max_id + 1
// int32 per row; score_bytes 0 = the default budget, a negative one = one row.
constexpr int64_t kRankedRowsBudget = int64_t(256) << 20;
int32_t ranked_groups(int32_t nq, int64_t slots, int64_t score_bytes);

}  // namespace swplan
