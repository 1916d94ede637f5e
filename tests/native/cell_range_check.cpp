// cell_range_check — swplan::cell_range (the constants and pattern range of
// the inter scan's biased cell) on the CPU.  Arguments: groups of four
// integers "min_s max_s go ge"; one line per group with the values
// tests/test_cell_range.py asserts on.  Linked from sw_plan.cpp alone.
#include <cstdio>
#include <cstdlib>

#include "sw_plan.h"

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) return 2;
    for (int k = 1; k + 3 < argc; k += 4) {
        const int min_s = std::atoi(argv[k]), max_s = std::atoi(argv[k + 1]), go = std::atoi(argv[k + 2]),
                  ge = std::atoi(argv[k + 3]);
        const swplan::CellRange c = swplan::cell_range(min_s, max_s, go, ge);
        std::printf("min_s %d max_s %d go %d ge %d: z %d sat_limit %d lowest %d guard %d top %d gog %08x diff %08x %08x %08x step",
                    min_s, max_s, go, ge, c.z, c.sat_limit, c.lowest, c.guard, c.top, c.gog, c.diff[0], c.diff[1],
                    c.diff[2]);
        for (uint32_t s : c.step) std::printf(" %08x", s);
        std::printf("\n");
    }
    std::printf("cell_range_check ok (cell %d..%d)\n", swplan::kCellMin, swplan::kCellMax);
    return 0;
}
