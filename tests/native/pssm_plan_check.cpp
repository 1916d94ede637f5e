// pssm_plan_check.cpp — swplan::plan_scoring_pssm on the CPU, linked from
// sw_plan.cpp alone (built and run by tests/test_pssm_cpu.py).
//
// A PSSM scan is planned from its table's entries: max_s and biased_fits come
// from plan_scoring_pssm, scan_plan is the sequence scan's.  One table on each
// side of each predicate of the scoring envelope:
//   max + go > 127                      a linear gap runs the affine kernels
//   2 max + 27 ge + go  against 1024    fp16 / int16, else int32
//   2 max + 39 ge + go  against 1024    20 rows per lane (long subjects only)
// and a table derived from a matrix (rows[i] = M[q[i]]) that contains the
// matrix's largest entry plans exactly as plan_scoring of that matrix.
#include <cstdio>
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

// nb blocks of widths wmax .. wmin, nlong long subjects of lengths lmax .. lmax / 2
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

// A table of qlen rows: `low` everywhere, `top` once (row `at`, column 17).
static std::vector<int8_t> table(int qlen, int low, int top, int at) {
    std::vector<int8_t> t(static_cast<size_t>(qlen) * 25, static_cast<int8_t>(low));
    t[static_cast<size_t>(at) * 25 + 17] = static_cast<int8_t>(top);
    return t;
}

static swplan::ScanPlan plan_pssm(const char* name, const Shape& sh, const std::vector<int8_t>& t, int go, int ge,
                                  int top) {
    const int qlen = static_cast<int>(t.size() / 25);
    const swplan::PlanScoring s = swplan::plan_scoring_pssm(t.data(), qlen, go, ge);
    CHECK(s.max_s == (top > 0 ? top : 0) && s.go == go && s.ge == ge && s.biased_fits == (top + go <= 127),
          "%s: max_s %d go %d ge %d biased_fits %d", name, s.max_s, s.go, s.ge, s.biased_fits);
    const swplan::ScanPlan p = swplan::scan_plan(sh.db, qlen, s, false, 0);
    std::printf("%s: %s | %s\n", name, p.kernel.c_str(), p.intra_kernel.c_str());
    return p;
}

static bool same(const swplan::PlanScoring& a, const swplan::PlanScoring& b) {
    return a.max_s == b.max_s && a.go == b.go && a.ge == b.ge && a.biased_fits == b.biased_fits;
}

int main() {
    const sw_opts o = policy_defaults();
    const Shape env(4, 1024, 40, 5, 1500, 1024, o);
    const Shape env_long(0, 0, 0, 150, 1500, 64, o);
    swplan::ScanPlan p;

    // max + go > 127: 100 + 27 fits the int8 linear profile, 100 + 28 does not
    p = plan_pssm("pssm-int8-fits-27", env, table(130, -50, 100, 129), 27, 27, 100);
    CHECK(!p.affine && p.f16, "int8 fits: %s", p.kernel.c_str());
    p = plan_pssm("pssm-int8-over-28", env, table(130, -50, 100, 0), 28, 28, 100);
    CHECK(p.affine && p.f16, "int8 over: %s", p.kernel.c_str());
    // ... by the largest entry, wherever it sits: 99 + 28 fits again
    p = plan_pssm("pssm-int8-fits-99-28", env, table(130, -50, 99, 64), 28, 28, 99);
    CHECK(!p.affine, "int8 fits at 99: %s", p.kernel.c_str());

    // 2 max + 27 ge + go: 1023 runs the 16-bit kernels, 1024 int32
    const struct { const char* name; int top, go, ge; bool fits; } rows[] = {
        {"pssm-big-go-974-1", 11, 974, 1, true},   {"pssm-big-go-975-1", 11, 975, 1, false},
        {"pssm-big-ge-191-30", 11, 191, 30, true}, {"pssm-big-ge-192-30", 11, 192, 30, false},
        {"pssm-big-linear-35", 15, 35, 35, true},  {"pssm-big-linear-36", 15, 36, 36, false},
        {"pssm-top-12-973-1", 12, 973, 1, false},  {"pssm-non-positive-12-1", 0, 12, 1, true}};
    for (const auto& r : rows) {
        p = plan_pssm(r.name, env, table(130, -4, r.top, 77), r.go, r.ge, r.top);
        const int sum = 2 * r.top + 27 * r.ge + r.go;
        CHECK((sum < 1024) == r.fits, "%s: sum %d", r.name, sum);
        CHECK(p.f16 == r.fits && p.intra_x2 == r.fits && (p.x2_ok != 0) == r.fits, "%s: f16 %d intra_x2 %d x2_ok %d",
              r.name, p.f16, p.intra_x2, p.x2_ok);
        CHECK(r.fits ? p.kernel.rfind("sw_inter_x2p<", 0) == 0 && p.intra_kernel.rfind("sw_intra_x2<", 0) == 0
                     : p.kernel.rfind("sw_inter<", 0) == 0 && p.intra_kernel.rfind("sw_intra<", 0) == 0 && !p.rescue,
              "%s: %s | %s", r.name, p.kernel.c_str(), p.intra_kernel.c_str());
    }
    // a table with no positive entry plans with max_s 0 (as a non-positive matrix)
    {
        const swplan::PlanScoring s = swplan::plan_scoring_pssm(table(40, -7, -3, 5).data(), 40, 12, 1);
        CHECK(s.max_s == 0 && s.biased_fits, "negative table: max_s %d", s.max_s);
    }

    // 2 max + 39 ge + go (long subjects only): 1023 takes 20 rows per lane, 1024 does not
    CHECK(swk::intra_bias_rows(swk::kIntraX2MaxRI) == 38 && 2 * 11 + 39 * 20 + 221 == 1023, "the wide rows are not at the bound");
    p = plan_pssm("pssm-long-wide-221-20", env_long, table(1280, -4, 11, 1279), 221, 20, 11);
    CHECK(p.ri2 == 20 && p.intra_kernel == "sw_intra_x2<20>", "wide 221/20: %s", p.intra_kernel.c_str());
    p = plan_pssm("pssm-long-wide-222-20", env_long, table(1280, -4, 11, 1279), 222, 20, 11);
    CHECK(p.ri2 != 20 && p.intra_x2, "wide 222/20: %s", p.intra_kernel.c_str());

    // derived tables: rows[i] = M[q[i]]
    int8_t m[625];
    for (int k = 0; k < 625; ++k) m[k] = static_cast<int8_t>(k / 25 == k % 25 ? 4 + k % 7 : -4 + k % 3);
    m[3 * 25 + 17] = 15;  // the largest entry: row 3
    for (int with_top = 0; with_top < 2; ++with_top) {
        std::vector<int8_t> t;
        for (int i = 0; i < 375; ++i) {
            int q = (7 * i + 1) % 25;
            if (q == 3 && !with_top) q = 4;
            t.insert(t.end(), m + 25 * q, m + 25 * q + 25);
        }
        for (const auto& g : {std::pair<int, int>{2, 2}, {12, 1}, {113, 113}, {975, 1}}) {
            const swplan::PlanScoring a = swplan::plan_scoring_pssm(t.data(), 375, g.first, g.second);
            const swplan::PlanScoring b = swplan::plan_scoring(m, g.first, g.second);
            if (with_top) {
                CHECK(same(a, b), "derived table with the top entry: go %d ge %d: max_s %d against %d", g.first, g.second,
                      a.max_s, b.max_s);
                const swplan::ScanPlan pa = swplan::scan_plan(env.db, 375, a, false, 0), pb = swplan::scan_plan(env.db, 375, b, false, 0);
                CHECK(pa.kernel == pb.kernel && pa.intra_kernel == pb.intra_kernel && pa.affine == pb.affine &&
                          pa.x2_ok == pb.x2_ok && pa.ri == pb.ri && pa.ri2 == pb.ri2 && pa.lpt == pb.lpt,
                      "derived table plans as its matrix: %s against %s", pa.kernel.c_str(), pb.kernel.c_str());
            } else {
                CHECK(a.max_s == 10 && a.max_s < b.max_s, "derived table without row 3: max_s %d", a.max_s);
            }
        }
    }
    // an empty table
    {
        const swplan::PlanScoring s = swplan::plan_scoring_pssm(nullptr, 0, 2, 2);
        CHECK(s.max_s == 0 && s.biased_fits, "empty table: max_s %d", s.max_s);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("pssm_plan_check ok\n");
    return 0;
}
