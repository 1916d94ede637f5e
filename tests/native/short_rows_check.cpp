// short_rows_check — swplan::short_rows (the rows per strip, Re, of the last
// pass of a two-strips scan) on the CPU: for every query length and both pass
// heights, Re is R or R - 4 (the kernels' two forms of a pass), the two strips
// hold the rows the query has left, the shorter form is taken wherever it
// would, and worked values.  Linked from sw_plan.cpp alone (tests/test_short_rows.py).
#include <cstdio>
#include <cstring>

#include "sw_plan.h"

static int failures = 0;
#define CHECK(c, ...)                  \
    do {                               \
        if (!(c)) {                    \
            std::printf(__VA_ARGS__);  \
            std::printf("\n");         \
            ++failures;                \
        }                              \
    } while (0)

int main() {
    for (int rows : {64, 96}) {
        const int R = rows / 2;
        for (int qlen = 1; qlen <= 4 * rows + 1; ++qlen) {
            const int re = swplan::short_rows(qlen, rows);
            const int s0 = (qlen - 1) / rows * rows;  // the last pass's first row
            CHECK(re == R || re == R - 4, "rows %d qlen %d: Re %d", rows, qlen, re);
            CHECK(s0 + 2 * re >= qlen, "rows %d qlen %d: Re %d leaves rows out", rows, qlen, re);
            CHECK(re == R - 4 || s0 + 2 * (R - 4) < qlen, "rows %d qlen %d: Re %d is not the smallest", rows, qlen, re);
        }
    }
    CHECK(swplan::short_rows(375, 64) == 28, "375 aa, 64-row passes");
    CHECK(swplan::short_rows(375, 96) == 44, "375 aa, 96-row passes");
    CHECK(swplan::short_rows(144, 64) == 28, "144 aa");
    CHECK(swplan::short_rows(64, 64) == 32 && swplan::short_rows(1, 64) == 28 && swplan::short_rows(65, 64) == 28 &&
              swplan::short_rows(56, 64) == 28 && swplan::short_rows(57, 64) == 32,
          "pass boundaries");
    // scan_plan passes it on for the two-strips shapes, at the launch's pass height
    // the library's choice for every policy (sw_opts_init's -1s; the checker links sw_plan.cpp alone)
    sw_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = static_cast<int32_t>(sizeof o);
    for (int32_t* f : {&o.lpt_pipe, &o.quad_width, &o.pair_width, &o.pair_group, &o.coop_width, &o.tail_pairs,
                       &o.tri_width, &o.lpt_pipe_tail, &o.lpt, &o.lpt_rows, &o.intra_x2, &o.intra_x2_rows,
                       &o.int16_guard})
        *f = -1;
    const uint32_t groups[4] = {40, 30, 20, 10};
    const int32_t llen[2] = {3000, 2000};
    swplan::PlanDb db;
    db.n = 4 * 64 + 2;
    db.residues = db.n * 300;
    db.nblocks = 4;
    db.nlong = 2;
    db.long_threshold = 1000;
    db.long_max = 3000;
    db.blk_groups = groups;
    db.llen = llen;
    db.opts = &o;
    db.cus = 256;
    for (int qlen : {1, 144, 375, 384, 385}) {
        for (int lin = 0; lin < 2; ++lin) {
            swplan::PlanScoring s;
            s.max_s = lin ? 15 : 11;
            s.go = lin ? 2 : 12;
            s.ge = lin ? 2 : 1;
            const swplan::ScanPlan p = swplan::scan_plan(db, qlen, s, false, 0);
            const int rows = p.lpt_rows == 96 ? 96 : 64;
            CHECK(p.shape.x2s && p.re_last == swplan::short_rows(qlen, rows) && p.qpad_inter % rows == 0,
                  "scan_plan qlen %d lin %d: re_last %d, %d-row passes", qlen, lin, p.re_last, rows);
        }
    }
    if (failures) return 1;
    std::printf("short_rows_check ok\n");
    return 0;
}
