// rank_check — the ranking by E-value's host half (csrc/sw_calib.cpp:
// rank_table, rank_min; sw_calib.h: rank_value, rank_key) alone, as its own
// program (built with -fsanitize=address,undefined by tests/test_rank_cpu.py):
// the adjustment table's fixed points, monotony, zeros and int32 saturation,
// the rank value's saturations and order, the key's order and id, and the
// cutoff's special cases and its agreement with the E-value formula.
//   rank_check : the checks; ends with "rank_check ok"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sw_calib.h"

static int g_fail = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                 \
            std::printf("\n");                        \
            ++g_fail;                                 \
        }                                             \
    } while (0)

using namespace swcalib;

static sw_calib make(double a, double c, double sigma, int64_t n_db, int status = 0) {
    sw_calib k{};
    k.size = static_cast<int32_t>(sizeof(sw_calib));
    k.status = status;
    k.qlen = 300;
    k.fits = 2;
    k.n_db = k.n_fit = n_db;
    k.a = a;
    k.c = c;
    k.sigma = sigma;
    return k;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- adj ------------------------------------------------------------------
    const int32_t max_len = 40000;
    std::vector<int32_t> adj(max_len + 1, -7);
    const sw_calib cal = make(19.6, 4.13, 6.2, 570000);
    rank_table(cal, max_len, adj.data());
    CHECK(adj[0] == 0 && adj[1] == 0, "adj[0], adj[1] = %d, %d", adj[0], adj[1]);
    for (int32_t L = 1; L <= max_len; ++L) {
        const long long want = std::llround(4096.0 * 4.13 * std::log(double(L)));
        CHECK(std::llabs(adj[L] - want) <= 1, "adj[%d] = %d, want %lld", L, adj[L], want);
        CHECK(L == 1 || adj[L] >= adj[L - 1], "adj not monotone at %d", L);
    }
    std::vector<int32_t> one(1, -7);  // max_len 0: one entry
    rank_table(cal, 0, one.data());
    CHECK(one[0] == 0, "adj of max_len 0");
    rank_table(make(20, 4, 0, 1000, SW_CALIB_DEGENERATE), max_len, adj.data());
    for (int32_t L = 0; L <= max_len; ++L) CHECK(adj[L] == 0, "degenerate adj[%d] = %d", L, adj[L]);
    rank_table(make(20, 1e6, 5, 1000), 100, adj.data());
    CHECK(adj[1] == 0 && adj[2] == INT32_MAX && adj[100] == INT32_MAX, "saturation up: %d %d", adj[2], adj[100]);
    rank_table(make(20, -1e6, 5, 1000), 100, adj.data());
    CHECK(adj[1] == 0 && adj[2] == INT32_MIN && adj[100] == INT32_MIN, "saturation down: %d %d", adj[2], adj[100]);

    // ---- the rank value and its key ------------------------------------------
    CHECK(kRankFloor == -4294967295LL && kRankCeil == 4294967295LL && kRankNone == 4294967296LL, "constants");
    CHECK(rank_value(0, 10, 0) == kRankFloor && rank_value(-1, 10, 0) == kRankFloor &&
              rank_value(INT32_MIN, 10, 5) == kRankFloor && rank_value(50, 0, 0) == kRankFloor, "floor cases");
    CHECK(rank_value(1, 1, 0) == 4096 && rank_value(100, 7, 1000) == 100 * 4096 - 1000, "plain values");
    CHECK(rank_value((1 << 20) - 1, 5, 0) == ((1LL << 20) - 1) * 4096 && rank_value(1 << 20, 5, 0) == ((1LL << 20) - 1) * 4096 &&
              rank_value(INT32_MAX, 5, 0) == ((1LL << 20) - 1) * 4096, "score clamp");
    CHECK(rank_value(INT32_MAX, 5, INT32_MIN) == kRankCeil, "upper saturation");
    CHECK(rank_value(1, 5, INT32_MAX) == 4096 - 2147483647LL, "largest adjustment");
    const int64_t lo = rank_key(kRankFloor, 0x7fffffff), hi = rank_key(kRankCeil, 0);
    CHECK(lo > INT64_MIN && hi > lo, "key range");
    CHECK(rank_key(5, 3) > rank_key(5, 4) && rank_key(6, 1000) > rank_key(5, 0) && rank_key(-5, 3) > rank_key(-6, 0), "key order");
    const int64_t rs[] = {kRankFloor, -4096, -1, 0, 1, 123456789, kRankCeil};
    const int32_t ids[] = {0, 1, 77, 0x7ffffffe, 0x7fffffff};
    for (int64_t r : rs)
        for (int32_t id : ids) CHECK(rank_key_id(rank_key(r, id)) == id, "id of key(%lld, %d)", (long long)r, id);

    // ---- the cutoff -----------------------------------------------------------
    int64_t r_min = 7;
    CHECK(!rank_min(cal, 0, &r_min) && !rank_min(cal, -1, &r_min) && !rank_min(cal, nan, &r_min), "invalid max_evalue");
    CHECK(rank_min(cal, inf, &r_min) && r_min == kRankFloor, "+inf");
    CHECK(rank_min(cal, 570000, &r_min) && r_min == kRankFloor, "max_evalue == n_db");
    CHECK(rank_min(cal, 1e9, &r_min) && r_min == kRankFloor, "max_evalue > n_db");
    const sw_calib deg = make(3, 0, 0, 1000, SW_CALIB_DEGENERATE);
    CHECK(rank_min(deg, 1000, &r_min) && r_min == kRankFloor, "degenerate, no cutoff");
    CHECK(rank_min(deg, 999, &r_min) && r_min == kRankNone, "degenerate, cutoff");
    CHECK(rank_min(make(3, 0, 0, 0), 5, &r_min) && r_min == kRankFloor, "empty database");
    // hand-made (s, L): at or above r_min E <= max_evalue (1 + 1e-3); two below, E > max_evalue (1 - 1e-3)
    rank_table(cal, max_len, adj.data());
    const double cut[] = {1e-30, 1e-6, 1e-3, 1, 10, 1000, 5e5, 569999.5};
    const int32_t Ls[] = {1, 2, 17, 100, 1000, 35213};
    for (double e : cut) {
        CHECK(rank_min(cal, e, &r_min) && r_min > kRankFloor && r_min < kRankNone, "r_min(%g)", e);
        int above = 0, below = 0;
        for (int32_t L : Ls)
            for (int32_t s = 1; s < 1400; ++s) {
                const int64_t r = rank_value(s, L, adj[L]);
                sw_sig g;
                significance(cal, s, L, &g);
                if (r >= r_min) {
                    ++above;
                    CHECK(g.evalue <= e * (1 + 1e-3), "E(%d, %d) = %.9g passes %g", s, L, g.evalue, e);
                } else if (r <= r_min - 2) {
                    ++below;
                    CHECK(g.evalue > e * (1 - 1e-3), "E(%d, %d) = %.9g fails %g", s, L, g.evalue, e);
                }
            }
        CHECK(above > 0 && below > 0, "cutoff %g: %d above, %d below", e, above, below);
    }
    // monotone in max_evalue
    int64_t prev = kRankNone;
    for (double e : cut) {
        rank_min(cal, e, &r_min);
        CHECK(r_min <= prev, "r_min not monotone at %g", e);
        prev = r_min;
    }
    if (g_fail) return 1;
    std::printf("rank_check ok\n");
    return 0;
}
