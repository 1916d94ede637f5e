// tests/native/batch_hits_check.cpp — CPU checks of the batched hit table's
// plan (built and run by tests/test_batch_hits_cpu.py), csrc/sw_plan.h:
//   cost    swplan::hits_cost against the bounds of sw_hits.hip's own loops,
//           restated here: per chunk, the blocks of slen + 63 steps plus two
//           rounds per further wave that holds a query row;
//   order   swplan::hits_order: a permutation, cost descending, stable;
//   groups  the per-hit swplan::hits_groups: within the budget unless a single
//           hit, never closed early, one-chunk hits free, and equal to the
//           single-qlen form on the same inputs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sw_kernels.h"
#include "sw_plan.h"

static int failures = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (failures < 20) {               \
                std::printf("FAIL: " __VA_ARGS__); \
                std::printf("\n");             \
            }                                  \
            ++failures;                        \
        }                                      \
    } while (0)

// The rounds of sw_hits.hip's `for (c0 ...) for (t ...)` loops for one hit.
static int64_t kernel_rounds(int64_t qlen, int64_t L) {
    if (qlen <= 0 || L <= 0) return 0;
    const int64_t W = swk::kHitsWaves, RI = swk::kHitsRowsPerLane, CH = swk::kHitsChunkRows, lanes = swk::kLanes;
    const int64_t nsteps = L + lanes - 1, nblk = (nsteps + lanes - 1) / lanes;
    int64_t rounds = 0;
    for (int64_t c0 = 0; c0 < qlen; c0 += CH) {
        const int64_t wact = std::min(W, (std::min(qlen - c0, CH) + lanes * RI - 1) / (lanes * RI));
        rounds += nblk + 2 * (wact - 1);
    }
    return rounds;
}

static void check_cost() {
    const int C = swk::kHitsChunkRows;
    int steps_q = 0, steps_s = 0;
    for (int q = 0; q <= 3 * C + 5; ++q)
        for (int64_t s : {int64_t(0), int64_t(1), int64_t(2), int64_t(64), int64_t(65), int64_t(66), int64_t(700), int64_t(35213)}) {
            CHECK(swplan::hits_cost(q, s) == kernel_rounds(q, s), "cost(%d, %lld) = %lld, the kernel runs %lld rounds", q,
                  (long long)s, (long long)swplan::hits_cost(q, s), (long long)kernel_rounds(q, s));
            if (q > 0) CHECK(swplan::hits_cost(q, s) >= swplan::hits_cost(q - 1, s), "not monotone in qlen at %d", q);
        }
    for (int q : {1, 129, C, C + 1, 2 * C + 3})
        for (int64_t s = 1; s <= 400; ++s) {
            CHECK(swplan::hits_cost(q, s) == kernel_rounds(q, s), "cost(%d, %lld)", q, (long long)s);
            CHECK(swplan::hits_cost(q, s) >= swplan::hits_cost(q, s - 1), "not monotone in slen at %lld", (long long)s);
            steps_s += swplan::hits_cost(q, s) > swplan::hits_cost(q, s - 1);
        }
    // a new chunk: its blocks again.  A new block of 64 steps: lane 63 ends a
    // subject of L columns at step L + 62, so blocks are added at L = 2, 66, 130, ...
    CHECK(swplan::hits_cost(C + 1, 100) > swplan::hits_cost(C, 100), "no step at qlen C -> C + 1");
    CHECK(swplan::hits_cost(C + 1, 100) - swplan::hits_cost(C, 100) == kernel_rounds(1, 100), "a chunk of one wave");
    CHECK(swplan::hits_cost(40, 66) == swplan::hits_cost(40, 65) + 1 && swplan::hits_cost(40, 65) == swplan::hits_cost(40, 2) &&
              swplan::hits_cost(40, 2) == swplan::hits_cost(40, 1) + 1,
          "blocks of 64 steps: one more at slen 2 and at slen 66");
    for (int q = 1; q <= C; ++q) steps_q += swplan::hits_cost(q, 100) > swplan::hits_cost(q - 1, 100);
    CHECK(steps_q == swk::kHitsWaves, "one step per wave within a chunk, %d", steps_q);
    CHECK(swplan::hits_cost(0, 100) == 0 && swplan::hits_cost(100, 0) == 0, "an empty pair costs nothing");
    std::printf("cost: C %lld rounds at slen 100, C+1 %lld, steps in slen 1..400 %d\n", (long long)swplan::hits_cost(C, 100),
                (long long)swplan::hits_cost(C + 1, 100), steps_s);
}

static void check_order() {
    const int C = swk::kHitsChunkRows;
    CHECK(swplan::hits_order(nullptr, nullptr, 0).empty(), "n = 0");
    std::mt19937 rng(11);
    int64_t ties = 0;
    for (int round = 0; round < 60; ++round) {
        const int64_t n = 1 + rng() % 300;
        std::vector<int32_t> ql(static_cast<size_t>(n));
        std::vector<int64_t> sl(static_cast<size_t>(n));
        for (int64_t k = 0; k < n; ++k) {
            ql[k] = static_cast<int32_t>(rng() % 8 == 0 ? 0 : rng() % (3 * C));
            sl[k] = rng() % 8 == 0 ? 0 : rng() % 900;
        }
        const std::vector<int64_t> order = swplan::hits_order(ql.data(), sl.data(), n);
        CHECK(static_cast<int64_t>(order.size()) == n, "order has n entries");
        std::vector<int> seen(static_cast<size_t>(n), 0);
        for (const int64_t k : order)
            if (k >= 0 && k < n) ++seen[k];
        CHECK(std::count(seen.begin(), seen.end(), 1) == n, "not a permutation");
        for (int64_t p = 1; p < n && static_cast<int64_t>(order.size()) == n; ++p) {
            const int64_t a = swplan::hits_cost(ql[order[p - 1]], sl[order[p - 1]]);
            const int64_t b = swplan::hits_cost(ql[order[p]], sl[order[p]]);
            CHECK(a >= b, "cost ascends at position %lld", (long long)p);
            if (a == b) {
                ++ties;
                CHECK(order[p - 1] < order[p], "equal costs out of the caller's order at %lld", (long long)p);
            }
        }
    }
    CHECK(ties > 100, "the inputs hold ties (%lld)", (long long)ties);
    std::printf("order: %lld ties kept in order\n", (long long)ties);
}

static void check_groups() {
    const int C = swk::kHitsChunkRows;
    const int64_t per = swplan::hits_scratch_bytes(C + 1, 1);
    std::mt19937 rng(7);
    int64_t multi = 0;
    for (int round = 0; round < 80; ++round) {
        const int64_t n = rng() % 60;
        const int64_t budget = per * (1 + rng() % 2000);
        std::vector<int64_t> slens(static_cast<size_t>(n));
        std::vector<int32_t> qlens(static_cast<size_t>(n));
        for (auto& s : slens) s = rng() % 10 == 0 ? 3000 + rng() % 3000 : rng() % 700;  // some alone over the budget
        for (auto& q : qlens) q = static_cast<int32_t>(rng() % 3 == 0 ? C + 1 + rng() % (2 * C) : rng() % (C + 1));
        const std::vector<int64_t> ends = swplan::hits_groups(qlens.data(), slens.data(), n, budget);
        CHECK((n == 0) == ends.empty() && (n == 0 || ends.back() == n), "groups end at n");
        int64_t k0 = 0;
        for (const int64_t k1 : ends) {
            CHECK(k1 > k0, "an empty group");
            int64_t bytes = 0;
            for (int64_t k = k0; k < k1; ++k) bytes += swplan::hits_scratch_bytes(qlens[k], slens[k]);
            CHECK(bytes <= budget || k1 == k0 + 1, "a group of %lld hits holds %lld bytes, budget %lld",
                  (long long)(k1 - k0), (long long)bytes, (long long)budget);
            if (k1 < n) CHECK(bytes + swplan::hits_scratch_bytes(qlens[k1], slens[k1]) > budget, "a group closed early");
            k0 = k1;
        }
        multi += ends.size() > 1;
        // a single repeated qlen: the existing function's result
        for (int q : {C, C + 1, 2 * C + 3}) {
            const std::vector<int32_t> same(static_cast<size_t>(n), q);
            CHECK(swplan::hits_groups(same.data(), slens.data(), n, budget) == swplan::hits_groups(q, slens.data(), n, budget),
                  "the per-hit form differs from the single-qlen form (q %d)", q);
        }
    }
    CHECK(multi > 20, "the inputs split into groups (%lld)", (long long)multi);
    // one-chunk hits are free: any number of them joins one group, around a multi-chunk hit too
    std::vector<int64_t> sl(5000, 100000);
    std::vector<int32_t> ql(5000, C);
    CHECK(swplan::hits_groups(ql.data(), sl.data(), 5000, per).size() == 1, "one-chunk hits count 0 bytes");
    ql[2500] = C + 1;
    sl[2500] = 1;
    CHECK(swplan::hits_groups(ql.data(), sl.data(), 5000, per).size() == 1, "... beside a multi-chunk hit that fits");
    ql[2501] = C + 1;
    sl[2501] = 1;
    const std::vector<int64_t> two = swplan::hits_groups(ql.data(), sl.data(), 5000, per);
    CHECK(two.size() == 2 && two[0] == 2501, "the second multi-chunk hit opens a group");
    std::printf("groups: %lld rounds split\n", (long long)multi);
}

int main() {
    check_cost();
    check_order();
    check_groups();
    std::printf(failures ? "batch_hits_check FAILED (%d)\n" : "batch_hits_check ok\n", failures);
    return failures ? 1 : 0;
}
