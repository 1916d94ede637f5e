// tests/native/plan_check.cpp — CPU check of the merged launch's work table
// (sw_plan.cpp lpt_plan) against the kernel's decoding of it
// (sw_inter_x2.hip x2p_wg and sw_scan_lpt, sw_intra_x2.h intra_x2_wg):
// every inter block and every long-subject pair is scanned by exactly one
// entry, whatever mix of quads / tri groups with spare waves / pairs /
// single waves / tail pairs and pipelined pairs the policies choose, and the
// table is sorted longest first.  And of the form of a scan (sw_plan.cpp
// scan_plan): the conditions every plan meets, and the forms of the scans
// whose routing is known, and one scoring on each side of every predicate
// of the scoring (plan_scoring on real matrices).  Built and run by
// tests/test_plan.py.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sw_kernels.h"
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

// one scenario: nb blocks of widths decreasing from wmax to wmin (16-column
// groups), nlong long subjects of lengths decreasing from lmax to lmax / 2
static void scenario(const char* name, int64_t nb, int wmax, int wmin, int64_t nlong, int lmax, int32_t npair,
                     int32_t nquad, int32_t ntail, bool affine, bool tri, int qlen, int rows, int ri, sw_opts o) {
    std::vector<uint32_t> groups(nb);
    for (int64_t b = 0; b < nb; ++b)
        groups[b] = static_cast<uint32_t>((wmax - (wmax - wmin) * b / (nb > 1 ? nb - 1 : 1) + 15) / 16);
    std::vector<int32_t> llen(nlong);
    for (int64_t k = 0; k < nlong; ++k) llen[k] = static_cast<int32_t>(lmax - (lmax / 2) * k / (nlong > 1 ? nlong - 1 : 1));
    swplan::PlanDb db;
    db.n = nb * 64 + nlong;
    db.residues = db.n * 300;
    db.nblocks = nb;
    db.nlong = nlong;
    db.long_threshold = lmax / 2;
    db.blk_groups = groups.data();
    db.llen = llen.data();
    db.opts = &o;
    db.cus = 256;
    const int32_t qpad = (qlen + rows - 1) / rows * rows;
    const int32_t qpad_intra = (qlen + 64 * ri - 1) / (64 * ri) * (64 * ri);
    const swplan::LptPlan p = swplan::lpt_plan(db, qpad, rows, qpad_intra, ri, npair, nquad, ntail, affine, tri);
    // the kernel's decoding (x2p_wg: MERGED, GMAX 4)
    const int64_t pwg = nquad + (npair - nquad + 1) / 2;
    const int64_t tail = ntail > 0 && nb - ntail > npair && nb - ntail < nb ? nb - ntail : nb;
    const bool tri_on = tri && affine;
    const int64_t nspare = tri_on ? std::max<int64_t>(0, std::min<int64_t>(nquad, tail - npair)) : 0;
    const int64_t s0 = npair + nspare;
    const int64_t twg = pwg + (tail - s0 + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    const int64_t npairs = (nlong + 1) / 2;
    const int64_t niwg = (npairs + swk::kWavesPerWG - 1) / swk::kWavesPerWG;
    std::vector<int> blk_seen(nb, 0), pair_seen(npairs, 0);
    std::vector<int> entry_seen(p.order.size() + 16, 0);
    for (size_t k = 0; k < p.order.size(); ++k) {
        const int32_t it = p.order[k];
        if (k) CHECK(p.cost[k] <= p.cost[k - 1], "%s: entry %zu out of order", name, k);
        if (it >= 0) {
            const int64_t wgi = it;
            if (wgi >= pwg && wgi < twg) {  // single waves
                for (int w = 0; w < swk::kWavesPerWG; ++w) {
                    const int64_t b = s0 + (wgi - pwg) * swk::kWavesPerWG + w;
                    if (b < tail) ++blk_seen[b];
                }
            } else if (wgi >= twg) {        // tail pairs: two blocks
                for (int q = 0; q < 2; ++q) {
                    const int64_t b = tail + (wgi - twg) * 2 + q;
                    if (b < nb) ++blk_seen[b];
                }
            } else if (wgi < nquad) {       // a quad or a tri (+ its spare's single)
                ++blk_seen[wgi];
                if (tri_on && npair + wgi < s0) ++blk_seen[npair + wgi];
            } else {                        // pairs: two blocks
                for (int q = 0; q < 2; ++q) {
                    const int64_t b = nquad + (wgi - nquad) * 2 + q;
                    if (b < npair) ++blk_seen[b];
                }
            }
        } else {
            const int64_t g = -1 - static_cast<int64_t>(it);
            if (g < niwg) {                 // an intra workgroup: pairs 4g .. 4g + 3, minus the pipelined
                for (int w = 0; w < swk::kWavesPerWG; ++w) {
                    const int64_t pr = g * swk::kWavesPerWG + w;
                    if (pr < npairs && pr >= p.npipe && pr < p.pipe_tail) ++pair_seen[pr];
                }
            } else {                        // a pipelined pair
                const int64_t pr = g - niwg;
                CHECK(pr >= 0 && pr < npairs, "%s: pipelined pair %lld out of range", name, (long long)pr);
                CHECK(pr < p.npipe || pr >= p.pipe_tail, "%s: pair %lld pipelined but not in a pipelined range", name,
                      (long long)pr);
                if (pr >= 0 && pr < npairs) ++pair_seen[pr];
            }
        }
    }
    for (int64_t b = 0; b < nb; ++b) CHECK(blk_seen[b] == 1, "%s: block %lld scanned %d times", name, (long long)b, blk_seen[b]);
    for (int64_t pr = 0; pr < npairs; ++pr)
        CHECK(pair_seen[pr] == 1, "%s: pair %lld scanned %d times", name, (long long)pr, pair_seen[pr]);
    std::printf("%s: %zu entries, npipe %d, pipe_tail %d of %lld pairs, spares %lld\n", name, p.order.size(), p.npipe,
                p.pipe_tail, (long long)npairs, (long long)nspare);
}

// the library's choice for every policy (sw_opts_init's -1s; the checker
// links sw_plan.cpp alone)
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

// ---- the form of a scan (sw_plan.cpp scan_plan) ----------------------------
// A database view of scenario()'s kind: nb blocks of widths wmax .. wmin,
// nlong long subjects of lengths lmax .. lmax / 2, long above `threshold`.
struct Shape {
    std::vector<uint32_t> groups;
    std::vector<int32_t> llen;
    sw_opts o;
    swplan::PlanDb db;
    Shape(int64_t nb, int wmax, int wmin, int64_t nlong, int lmax, int threshold, const sw_opts& opts)
        : groups(nb), llen(nlong), o(opts) {
        for (int64_t b = 0; b < nb; ++b)
            groups[b] = static_cast<uint32_t>((wmax - (wmax - wmin) * b / (nb > 1 ? nb - 1 : 1) + 15) / 16);
        for (int64_t k = 0; k < nlong; ++k)
            llen[k] = static_cast<int32_t>(lmax - (lmax / 2) * k / (nlong > 1 ? nlong - 1 : 1));
        db.n = nb * 64 + nlong;
        db.residues = db.n * 300;
        db.nblocks = nb;
        db.nlong = nlong;
        db.long_threshold = threshold;
        db.long_max = nlong ? lmax : 0;
        db.blk_groups = groups.data();
        db.llen = llen.data();
        db.opts = &o;
        db.cus = 256;
    }
    Shape(const Shape&) = delete;
};

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

// The plan of one scan, after the conditions every plan meets.
static swplan::ScanPlan plan(const char* name, const Shape& sh, int qlen, int max_s, int go, int ge,
                             bool i16_first = false, int32_t span = 0) {
    swplan::PlanScoring s;
    s.max_s = max_s;
    s.go = go;
    s.ge = ge;
    s.biased_fits = max_s + go <= 127;
    const swplan::ScanPlan p = swplan::scan_plan(sh.db, qlen, s, i16_first, span);
    // every padded length is a multiple of its kernel's pass height and holds the query
    const int heights[6][2] = {{p.qpad_inter, p.lpt_rows == 96 ? 96 : p.shape.R},
                               {p.qpad_intra, 64 * p.ri},
                               {p.qpad_intra2, 64 * p.ri2},
                               {p.qpad_rescue, swplan::rescue_rows(p.affine)},
                               {p.qpad_list, p.affine ? 64 : 96},
                               {p.qpad_coop, swk::kCoopRows}};
    for (int k = 0; k < 6; ++k) {
        const int q = heights[k][0], rows = heights[k][1];
        if (q == 0 && k != 0) continue;  // the kernel does not run
        CHECK(rows > 0 && q % rows == 0 && q >= qlen, "%s: padded length %d: %d for %d rows, qlen %d", name, k, q, rows, qlen);
    }
    CHECK((p.ri != 0) == (sh.db.nlong != 0), "%s: ri %d with %lld long subjects", name, p.ri, (long long)sh.db.nlong);
    CHECK((p.ri2 != 0) == p.intra_x2, "%s: ri2 %d, intra_x2 %d", name, p.ri2, p.intra_x2);
    CHECK((p.qpad_rescue != 0) == p.rescue && (p.qpad_list != 0) == p.f16 && (p.qpad_coop != 0) == (p.ncoop != 0),
          "%s: a padded length without its kernel", name);
    CHECK(!p.drain, "%s: draining before set_drain", name);
    if (p.lpt) {
        CHECK(p.npair > 0 && p.ncoop == 0 && p.nr == 0, "%s: lpt with npair %d ncoop %d nr %d", name, p.npair, p.ncoop, p.nr);
        CHECK(p.ri2 == 4 || p.ri2 == 6 || p.ri2 == 8, "%s: lpt with ri2 %d", name, p.ri2);
        CHECK(p.nquad <= p.npair && p.ntail < sh.db.nblocks - p.npair + (p.ntail == 0), "%s: lpt block ranges", name);
    } else {
        CHECK(!p.ntri && !p.nquad && !p.ntail && p.lpt_rows == 64, "%s: merged-launch fields without lpt", name);
    }
    CHECK(has(p.kernel, "+lpt") == p.lpt, "%s: name %s, lpt %d", name, p.kernel.c_str(), p.lpt);
    CHECK((p.lpt_rows == 96) == (p.lpt && !p.affine && qlen > 96), "%s: %d-row passes", name, p.lpt_rows);
    CHECK(has(p.kernel, "<48,") == (p.lpt_rows == 96), "%s: name %s, %d-row passes", name, p.kernel.c_str(), p.lpt_rows);
    CHECK(!p.ntri || (p.affine && p.nquad == p.ntri), "%s: ntri %d, affine %d, nquad %d", name, p.ntri, p.affine, p.nquad);
    CHECK(p.kernel.empty() == (sh.db.nblocks == 0), "%s: inter name '%s'", name, p.kernel.c_str());
    CHECK((p.intra_kernel == "none") == (sh.db.nlong == 0), "%s: intra name '%s'", name, p.intra_kernel.c_str());
    // set_drain: the int32 long-subject stage at the fp16 form's rows, the name's suffix, nothing else
    swplan::ScanPlan d = p;
    d.set_drain(true);
    CHECK(d.drain == p.lpt, "%s: set_drain(true) drains %d, lpt %d", name, d.drain, p.lpt);
    if (d.drain) {
        CHECK(d.ri == d.ri2 && d.qpad_intra == d.qpad_intra2, "%s: drain ri %d ri2 %d", name, d.ri, d.ri2);
        CHECK(d.kernel == p.kernel + "+drain", "%s: drain name %s", name, d.kernel.c_str());
        d.ri = p.ri;
        d.qpad_intra = p.qpad_intra;
        d.multi_intra = p.multi_intra;
        d.kernel = p.kernel;
        d.drain = false;
    }
    swplan::ScanPlan e = p;
    e.set_drain(false);
    for (const swplan::ScanPlan* q : {&d, &e})
        CHECK(q->ri == p.ri && q->ri2 == p.ri2 && q->qpad_inter == p.qpad_inter && q->qpad_intra == p.qpad_intra &&
                  q->qpad_intra2 == p.qpad_intra2 && q->npair == p.npair && q->ntri == p.ntri && q->nquad == p.nquad &&
                  q->ntail == p.ntail && q->lpt == p.lpt && q->lpt_rows == p.lpt_rows && q->kernel == p.kernel &&
                  q->intra_kernel == p.intra_kernel && q->multi_inter == p.multi_inter && !q->drain,
              "%s: set_drain changed more than ri, qpad_intra and the name", name);
    std::printf("%s: %s | %s ri %d ri2 %d\n", name, p.kernel.c_str(), p.intra_kernel.c_str(), p.ri, p.ri2);
    return p;
}

// The forms below are what the scan driver chose before scan_plan existed
// (read off that code, not off sw_plan.cpp).
static void scan_forms(const sw_opts& o) {
    const int kB62 = 11, kB50 = 15;  // the largest entries of BLOSUM62 and of the reference's BLOSUM50
    // C2's 1/8 share shape: 1,065 blocks up to 891 columns, 3,122 long subjects
    const Shape share8(1065, 891, 32, 3122, 7429, 891, o);
    swplan::ScanPlan p = plan("share8-affine-q375", share8, 375, kB62, 12, 1);
    CHECK(p.affine && p.x2_ok == 2 && p.lpt && p.ri2 == 6 && p.ntri > 0 && has(p.kernel, "+tri"), "share8 affine: %s", p.kernel.c_str());
    CHECK(p.kernel.rfind("sw_inter_x2p<32,8,affine,fp16>", 0) == 0 && p.intra_kernel == "sw_intra_x2<6>", "share8 affine names");
    p = plan("share8-linear-q375", share8, 375, kB50, 2, 2);
    CHECK(!p.affine && p.lpt && p.lpt_rows == 96 && p.qpad_inter == 384 && p.ntri == 0, "share8 linear 375: %s", p.kernel.c_str());
    CHECK(p.kernel.rfind("sw_inter_x2p<48,8,linear,fp16>", 0) == 0, "share8 linear 375: %s", p.kernel.c_str());
    p = plan("share8-linear-q96", share8, 96, kB50, 2, 2);
    CHECK(p.lpt && p.lpt_rows == 64 && p.qpad_inter == 128, "share8 linear 96: %s", p.kernel.c_str());
    CHECK(p.kernel.rfind("sw_inter_x2p<32,8,linear,fp16>", 0) == 0, "share8 linear 96: %s", p.kernel.c_str());
    p = plan("share8-linear-q97", share8, 97, kB50, 2, 2);
    CHECK(p.lpt && p.lpt_rows == 96 && p.qpad_inter == 192, "share8 linear 97: %s", p.kernel.c_str());
    // one pass of the two-strips kernel: no pair form, so no merged launch
    for (int qlen : {1, 40, 64})
        for (int lin = 0; lin < 2; ++lin) {
            p = plan("share8-one-pass", share8, qlen, lin ? kB50 : kB62, lin ? 2 : 12, lin ? 2 : 1);
            CHECK(!p.lpt && p.npair == 0 && p.ncoop == 0 && p.qpad_inter == 64, "one pass: qlen %d: %s", qlen, p.kernel.c_str());
            CHECK(p.kernel == (lin ? "sw_inter_x2s<32,8,linear,fp16>" : "sw_inter_x2s<32,8,affine,fp16>"), "one pass: %s", p.kernel.c_str());
        }
    // a long query: the cost model wants 12 rows per lane; affine scans take
    // the merged launch at 8 instead, unless it is off; linear ones keep 12
    p = plan("share8-affine-q1400", share8, 1400, kB62, 12, 1);
    CHECK(p.lpt && p.ri2 == 8 && p.qpad_intra2 == 1536, "affine 1400: ri2 %d %s", p.ri2, p.kernel.c_str());
    {
        sw_opts off = o;
        off.lpt = 0;
        const Shape s2(1065, 891, 32, 3122, 7429, 891, off);
        p = plan("share8-affine-q1400-lpt0", s2, 1400, kB62, 12, 1);
        CHECK(!p.lpt && p.ri2 == 12 && p.qpad_intra2 == 1536 && p.intra_kernel == "sw_intra_x2<12>", "affine 1400, lpt 0: ri2 %d", p.ri2);
        CHECK(p.kernel == "sw_inter_x2p<32,8,affine,fp16>", "affine 1400, lpt 0: %s", p.kernel.c_str());
        p = plan("share8-affine-q375-lpt0", s2, 375, kB62, 12, 1);
        CHECK(!p.lpt && p.ri2 == 6 && p.kernel == "sw_inter_x2p<32,8,affine,fp16>", "affine 375, lpt 0: %s", p.kernel.c_str());
    }
    p = plan("share8-linear-q1400", share8, 1400, kB50, 2, 2);
    CHECK(!p.lpt && p.ri2 == 12, "linear 1400: ri2 %d %s", p.ri2, p.kernel.c_str());
    // the adaptive routes: a span of int16 blocks, int16 first over the long subjects
    p = plan("share8-span5", share8, 375, kB50, 2, 2, false, 5);
    CHECK(!p.lpt && p.nr == 5 && p.kernel == "sw_inter_x2p<32,8,linear,fp16>+int16[0,5)", "span 5: %s", p.kernel.c_str());
    p = plan("share8-span5-one-pass", share8, 40, kB50, 2, 2, false, 5);
    CHECK(!p.lpt && p.nr == 0 && p.kernel == "sw_inter_x2s<32,8,linear,fp16>", "span 5, one pass: %s", p.kernel.c_str());
    p = plan("share8-i16-first", share8, 375, kB50, 2, 2, true, 0);
    CHECK(!p.lpt && p.intra_i16_first && p.intra_kernel == "sw_intra_x2<6,int16>", "int16 first: %s", p.intra_kernel.c_str());
    // beyond the static int16 bound: guarded; scales the fp16 cell cannot hold: int32 only
    p = plan("share8-guarded", share8, 2000, kB62, 12, 1);
    CHECK(p.x2_ok == 1 && p.shape.x2s && p.rescue, "guarded: x2_ok %d %s", p.x2_ok, p.kernel.c_str());
    p = plan("share8-int32-affine", share8, 375, kB62, 120, 120);  // S + gap leaves the int8 profile too
    CHECK(p.affine && p.x2_ok == 0 && !p.intra_x2 && !p.rescue && p.kernel == "sw_inter<32,8,affine>", "int32 affine: %s", p.kernel.c_str());
    CHECK(p.intra_kernel.rfind("sw_intra<", 0) == 0 && has(p.intra_kernel, ",affine>"), "int32 affine: %s", p.intra_kernel.c_str());
    p = plan("share8-int32-linear", share8, 375, kB62, 40, 40);
    CHECK(!p.affine && p.x2_ok == 0 && p.kernel == "sw_inter<64,8,linear>" && has(p.intra_kernel, ",linear>"), "int32 linear: %s", p.kernel.c_str());
    // 20 rows per lane: only without inter blocks (no merged launch could take the scan), affine gaps
    const Shape only_long(0, 0, 0, 500, 4000, 64, o);
    p = plan("only-long-affine-q1280", only_long, 1280, kB62, 12, 1);
    CHECK(p.ri2 == 20 && p.intra_kernel == "sw_intra_x2<20>" && p.kernel.empty() && !p.lpt, "only long: ri2 %d", p.ri2);
    p = plan("only-long-linear-q1280", only_long, 1280, kB50, 2, 2);
    CHECK(p.ri2 != 20, "only long, linear: ri2 %d", p.ri2);
    for (int qlen : {200, 1280, 2560, 5000})
        for (int lin = 0; lin < 2; ++lin) {
            p = plan("share8-never-20", share8, qlen, lin ? kB50 : kB62, lin ? 2 : 12, lin ? 2 : 1);
            CHECK(p.ri2 != 20, "with blocks: qlen %d ri2 %d", qlen, p.ri2);
        }
    // no long subjects: no merged launch, whatever sw_opts lpt says
    sw_opts on = o;
    on.lpt = 1;
    const Shape only_short(300, 700, 16, 0, 0, 700, on);
    p = plan("only-short", only_short, 375, kB62, 12, 1);
    CHECK(!p.lpt && p.npair > 0 && p.ri == 0 && p.intra_kernel == "none", "only short: %s", p.kernel.c_str());
}

// ---- the scoring predicates (sw_plan.cpp plan_scoring + scan_plan) ---------
// A real 625-entry matrix: `off` everywhere, `diag` on the diagonal, and one
// off-diagonal entry (row 3, column 17) holding the largest value `top`.
struct Matrix {
    int8_t m[625];
    Matrix(int diag, int off, int top) {
        for (int k = 0; k < 625; ++k) m[k] = static_cast<int8_t>(k / 25 == k % 25 ? diag : off);
        m[3 * 25 + 17] = static_cast<int8_t>(top);
    }
};

// plan()'s checks and line for a scan whose PlanScoring the library's own
// plan_scoring filled from the matrix.
static swplan::ScanPlan plan_real(const char* name, const Shape& sh, int qlen, const Matrix& mx, int go, int ge) {
    const swplan::PlanScoring s = swplan::plan_scoring(mx.m, go, ge);
    int top = 0;
    for (int k = 0; k < 625; ++k) top = std::max<int>(top, mx.m[k]);
    CHECK(s.max_s == top && s.go == go && s.ge == ge && s.biased_fits == (top + go <= 127),
          "%s: plan_scoring max_s %d go %d ge %d biased_fits %d", name, s.max_s, s.go, s.ge, s.biased_fits);
    return plan(name, sh, qlen, s.max_s, go, ge);
}

// One row on each side of each predicate of the scoring that switches kernel
// families.  The database views: a few inter blocks beside a few long
// subjects (tests/test_gpu_scoring_envelope.py scans one of that shape and
// asserts the same names), and long subjects only.
static void scoring_thresholds(const sw_opts& o) {
    const Shape env(4, 1024, 40, 5, 1500, 1024, o);
    const Shape env_long(0, 0, 0, 150, 1500, 64, o);
    const Matrix m100(100, -50, 100), m11(4, -4, 11), m15(5, -5, 15), m0(-1, -3, 0);
    swplan::ScanPlan p;
    // biased_fits: S + gap = 127 is the int8 linear profile's last value
    p = plan_real("env-int8-fits-27", env, 130, m100, 27, 27);
    CHECK(!p.affine && p.f16 && p.kernel.rfind("sw_inter_x2p<48,8,linear,fp16>", 0) == 0, "int8-fits: %s", p.kernel.c_str());
    p = plan_real("env-int8-over-28", env, 130, m100, 28, 28);
    CHECK(p.affine && p.f16 && p.kernel.rfind("sw_inter_x2p<32,8,affine,fp16>", 0) == 0, "int8-over: %s", p.kernel.c_str());
    {
        const swplan::PlanScoring s = swplan::plan_scoring(m100.m, 28, 28);
        CHECK(s.go == s.ge && !s.biased_fits, "int8-over: go %d ge %d biased_fits %d", s.go, s.ge, s.biased_fits);
    }
    // f16_fits: 2 max S + 27 ge + go at 1023 and 1024, by a large open, a large extend, a linear gap
    const struct { const char* name; const Matrix* mx; int go, ge; bool fits; const char* i32; } rows[] = {
        {"env-big-go-974-1", &m11, 974, 1, true, ""},    {"env-big-go-975-1", &m11, 975, 1, false, "sw_inter<32,8,affine>"},
        {"env-big-ge-191-30", &m11, 191, 30, true, ""},  {"env-big-ge-192-30", &m11, 192, 30, false, "sw_inter<32,8,affine>"},
        {"env-big-linear-35", &m15, 35, 35, true, ""},   {"env-big-linear-36", &m15, 36, 36, false, "sw_inter<64,8,linear>"},
        {"env-non-positive-12-1", &m0, 12, 1, true, ""}, {"env-limits-1000-1000", &m100, 1000, 1000, false, "sw_inter<32,8,affine>"}};
    for (const auto& r : rows) {
        p = plan_real(r.name, env, 130, *r.mx, r.go, r.ge);
        const int sum = 2 * swplan::plan_scoring(r.mx->m, r.go, r.ge).max_s + 27 * r.ge + r.go;
        CHECK((sum < 1024) == r.fits, "%s: sum %d", r.name, sum);
        CHECK(p.f16 == r.fits && p.intra_x2 == r.fits && (p.x2_ok != 0) == r.fits, "%s: f16 %d intra_x2 %d x2_ok %d", r.name,
              p.f16, p.intra_x2, p.x2_ok);
        if (r.fits)
            CHECK(p.kernel.rfind(r.go == r.ge ? "sw_inter_x2p<48,8,linear,fp16>" : "sw_inter_x2p<32,8,affine,fp16>", 0) == 0 &&
                      p.intra_kernel.rfind("sw_intra_x2<", 0) == 0, "%s: %s | %s", r.name, p.kernel.c_str(), p.intra_kernel.c_str());
        else
            CHECK(p.kernel == r.i32 && p.intra_kernel.rfind("sw_intra<", 0) == 0 && !p.rescue, "%s: %s | %s", r.name,
                  p.kernel.c_str(), p.intra_kernel.c_str());
    }
    // the sums themselves: 1023 fits, 1024 does not
    CHECK(2 * 11 + 27 * 1 + 974 == 1023 && 2 * 11 + 27 * 30 + 191 == 1023 && 2 * 15 + 28 * 35 == 1010 && 2 * 15 + 28 * 36 == 1038,
          "the f16_fits rows are not at the bound");
    // x2_ok 2 against 1: (qlen + 2) (max S + go) = 32,766 = 258 x 127 and 32,767 = 217 x 151;
    // without the guard (sw_opts int16_guard 0) the second is an int32 scan
    sw_opts ng = o;
    ng.int16_guard = 0;
    const Shape env_ng(4, 1024, 40, 5, 1500, 1024, ng);
    p = plan_real("env-static-32766", env, 256, m11, 116, 1);
    CHECK(p.x2_ok == 2 && p.f16, "32766: x2_ok %d", p.x2_ok);
    p = plan_real("env-static-32766-guard0", env_ng, 256, m11, 116, 1);
    CHECK(p.x2_ok == 2 && p.kernel.rfind("sw_inter_x2p<32,8,affine,fp16>", 0) == 0, "32766, guard 0: %s", p.kernel.c_str());
    p = plan_real("env-static-32767", env, 215, m11, 140, 1);
    CHECK(p.x2_ok == 1 && p.f16 && p.rescue, "32767: x2_ok %d", p.x2_ok);
    p = plan_real("env-static-32767-guard0", env_ng, 215, m11, 140, 1);
    CHECK(p.x2_ok == 1 && p.kernel == "sw_inter<32,8,affine>" && !p.rescue, "32767, guard 0: %s", p.kernel.c_str());
    p = plan_real("env-static-32893", env, 257, m11, 116, 1);
    CHECK(p.x2_ok == 1, "32893: x2_ok %d", p.x2_ok);
    // ri2_wide (long subjects only): 2 max S + (intra_bias_rows(20) + 1) ge + go at 1023 and 1024
    CHECK(swk::intra_bias_rows(swk::kIntraX2MaxRI) == 38 && 2 * 11 + 39 * 20 + 221 == 1023, "the ri2_wide rows are not at the bound");
    p = plan_real("long-wide-221-20", env_long, 1280, m11, 221, 20);
    CHECK(p.ri2 == 20 && p.intra_kernel == "sw_intra_x2<20>", "wide 221/20: %s", p.intra_kernel.c_str());
    p = plan_real("long-wide-222-20", env_long, 1280, m11, 222, 20);
    CHECK(p.ri2 != 20 && p.intra_x2 && p.intra_kernel.rfind("sw_intra_x2<", 0) == 0, "wide 222/20: %s", p.intra_kernel.c_str());
    sw_opts f20 = o;
    f20.intra_x2_rows = 20;  // forced: 20 rows only inside the bound
    const Shape env_long20(0, 0, 0, 150, 1500, 64, f20);
    p = plan_real("long-forced20-221-20", env_long20, 375, m11, 221, 20);
    CHECK(p.ri2 == 20, "forced 20, 221/20: ri2 %d", p.ri2);
    p = plan_real("long-forced20-222-20", env_long20, 375, m11, 222, 20);
    CHECK(p.ri2 != 20 && p.ri2 > 0, "forced 20, 222/20: ri2 %d", p.ri2);
    // ... and never beside inter blocks
    const Shape env20(4, 1024, 40, 5, 1500, 1024, f20);
    p = plan_real("env-forced20-12-1", env20, 375, m11, 12, 1);
    CHECK(p.ri2 != 20 && p.ri2 > 0, "forced 20 with blocks: ri2 %d", p.ri2);
}

int main() {
    const sw_opts o = policy_defaults();
    // C2's 1/8 share shape: 1,065 blocks, 3,122 long subjects, 375-aa query
    scenario("share8-affine-tri", 1065, 891, 32, 3122, 7429, 633, 275, 0, true, true, 375, 64, 6, o);
    scenario("share8-affine-quads", 1065, 891, 32, 3122, 7429, 633, 105, 0, true, false, 375, 64, 6, o);
    scenario("share8-linear-tailpipe", 1065, 891, 32, 3122, 7429, 633, 105, 0, false, false, 375, 96, 6, o);
    // more tris than single blocks: spares run out
    scenario("tris-exceed-singles", 200, 800, 100, 40, 2000, 190, 190, 0, true, true, 375, 64, 6, o);
    // tail pairs beside tris
    scenario("tris-and-tail-pairs", 2000, 1500, 16, 500, 4000, 600, 100, 256, true, true, 300, 64, 4, o);
    // a tail-pair count reaching into the group blocks: the kernel runs none
    scenario("tail-pairs-clamped", 300, 900, 48, 80, 3000, 250, 20, 100, true, true, 375, 64, 6, o);
    // forced pipes at both ends, odd long count
    sw_opts f = o;
    f.lpt_pipe = 3;
    f.lpt_pipe_tail = 37;
    scenario("pipes-both-ends", 500, 900, 48, 301, 5000, 300, 50, 64, true, true, 375, 64, 6, f);
    f.lpt_pipe_tail = 100000;  // every pair pipelined
    scenario("every-pair-pipelined", 300, 700, 48, 120, 3000, 150, 0, 0, false, false, 200, 64, 4, f);
    // no long subjects, no groups
    scenario("inter-only", 50, 300, 16, 0, 0, 0, 0, 0, true, false, 375, 64, 6, o);
    scan_forms(o);
    scoring_thresholds(o);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("plan_check ok\n");
    return 0;
}
