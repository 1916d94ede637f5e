// rank_groups_check — swplan::ranked_groups (csrc/sw_plan.cpp) alone: prints
// "nq slots score_bytes G" for every case tests/test_rank_cpu.py compares with
// its restatement (budgets below one row, exactly two rows, more than nq
// rows, the default), then "rank_groups_check ok".
#include <cstdio>

#include "sw_plan.h"

int main() {
    const int64_t slots = 901;  // a row of 3,604 bytes
    const int32_t nqs[] = {0, 1, 5};
    const int64_t budgets[] = {-1, 1, 4 * slots - 1, 4 * slots, 8 * slots - 1, 8 * slots, 8 * slots + 3, 20 * slots,
                               24 * slots, int64_t(1) << 40, 0};
    for (int32_t nq : nqs)
        for (int64_t b : budgets)
            std::printf("%d %lld %lld %d\n", nq, (long long)slots, (long long)b, swplan::ranked_groups(nq, slots, b));
    // the default budget on C2's shape (570,000 slots: 2.3 MB a row, 117 rows) and with no slots at all
    std::printf("%d %lld %lld %d\n", 1000, 570000LL, 0LL, swplan::ranked_groups(1000, 570000, 0));
    std::printf("%d %lld %lld %d\n", 7, 0LL, 0LL, swplan::ranked_groups(7, 0, 0));
    std::printf("rank_groups_check ok\n");
    return 0;
}
