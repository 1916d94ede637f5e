// calib_check — the calibration's host half (csrc/sw_calib.cpp) alone, as its
// own program (built with -fsanitize=address,undefined by
// tests/test_calib_cpu.py): the length bin's examples, range and monotony,
// the edge tables' status bits, a regression it can verify in closed form,
// and the significance formula's limits.
//   calib_check        : the checks; ends with "calib_check ok"
//   calib_check bins   : "L bin" for every L the Python test compares
#include <cmath>
#include <cstdio>
#include <cstring>
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

using swcalib::kCells;
using swcalib::kLBins;
using swcalib::kSBins;

static bool near(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "bins")) {
        for (uint32_t L = 1; L <= 70000; ++L) std::printf("%u %d\n", L, swcalib::length_bin(L));
        for (int k = 2; k <= 30; ++k) {
            const uint32_t p = 1u << k;
            const uint32_t v[3] = {p - 1, p, 5 * (p >> 2)};
            for (uint32_t L : v) std::printf("%u %d\n", L, swcalib::length_bin(L));
        }
        std::printf("%u %d\n", 0x7fffffffu, swcalib::length_bin(0x7fffffffu));
        return 0;
    }

    // ---- the bin ------------------------------------------------------------
    const int ex_L[] = {1, 2, 3, 4, 5, 7, 8}, ex_b[] = {0, 4, 6, 8, 9, 11, 12};
    for (int i = 0; i < 7; ++i) CHECK(swcalib::length_bin(ex_L[i]) == ex_b[i], "bin(%d) = %d", ex_L[i], swcalib::length_bin(ex_L[i]));
    int prev = 0;
    for (uint32_t L = 1; L < (1u << 20); ++L) {
        const int b = swcalib::length_bin(L);
        CHECK(b >= prev && b < 124, "bin(%u) = %d after %d", L, b, prev);
        prev = b;
    }
    CHECK(swcalib::length_bin(0x7fffffffu) == 123, "bin(2^31 - 1) = %d", swcalib::length_bin(0x7fffffffu));
    // a bin's abscissa lies inside the bin's length range
    for (uint32_t L = 4; L < 100000; L += 7) {
        const double x = swcalib::bin_abscissa(swcalib::length_bin(L));
        CHECK(std::fabs(x - std::log(double(L))) < std::log(1.25), "abscissa of bin(%u)", L);
    }
    CHECK(swcalib::score_bin(-5) == 0 && swcalib::score_bin(510) == 510 && swcalib::score_bin(511) == 511 &&
              swcalib::score_bin(512) == 511 && swcalib::score_bin(0x7fffffff) == 511, "score columns");

    // ---- edge tables ----------------------------------------------------------
    std::vector<uint32_t> H(kCells, 0);
    sw_calib c;
    sw_sig s;
    swcalib::fit(H.data(), 100, &c);
    CHECK((c.status & SW_CALIB_DEGENERATE) && (c.status & SW_CALIB_FEW) && c.n_db == 0 && c.fits == 0 && c.a == 0 &&
              c.c == 0 && c.sigma == 0 && c.size == (int)sizeof(sw_calib), "all-zero table: status %d", c.status);
    swcalib::significance(c, 50, 300, &s);
    CHECK(s.evalue == 0 && s.bits == 0 && s.z == 0, "all-zero table: E %g", s.evalue);

    H[33 * kSBins + 20] = 400;  // one bin, several scores
    H[33 * kSBins + 30] = 400;
    swcalib::fit(H.data(), 100, &c);
    CHECK((c.status & SW_CALIB_DEGENERATE) && c.n_db == 800 && c.n_fit == 800 && c.a == 25 && c.c == 0, "one bin: status %d a %g", c.status, c.a);
    swcalib::significance(c, 50, 300, &s);
    CHECK(s.evalue == 800 && s.bits == 0, "degenerate E %g bits %g", s.evalue, s.bits);

    std::fill(H.begin(), H.end(), 0);
    for (int b = 20; b < 50; ++b) H[b * kSBins + 37] = 100;  // one score everywhere
    swcalib::fit(H.data(), 100, &c);
    CHECK((c.status & SW_CALIB_DEGENERATE) && !(c.status & SW_CALIB_FEW) && c.a == 37 && c.sigma == 0 && c.n_fit == 3000, "one score: status %d a %g", c.status, c.a);

    std::fill(H.begin(), H.end(), 0);
    for (int b = 20; b < 50; ++b) H[b * kSBins + kSBins - 1] = 100;  // everything clipped
    swcalib::fit(H.data(), 100, &c);
    CHECK((c.status & SW_CALIB_DEGENERATE) && (c.status & SW_CALIB_CLIPPED) && c.n_clipped == 3000 && c.n_fit == 0, "all clipped: status %d", c.status);

    // ---- a regression in closed form -----------------------------------------
    // two scores per bin, round(10 + 4 x_b) -+ 3 with equal weights: the fit is
    // the regression of round(10 + 4 x_b) on x_b; the rounding keeps |r| < 4
    std::fill(H.begin(), H.end(), 0);
    double Sx = 0, Sy = 0, Sxx = 0, Sxy = 0;
    int nb = 0;
    for (int b = 16; b < 60; ++b) {
        const double x = swcalib::bin_abscissa(b);
        const int y = (int)std::lround(10 + 4 * x);
        H[b * kSBins + y - 3] = 50;
        H[b * kSBins + y + 3] = 50;
        Sx += x, Sy += y, Sxx += x * x, Sxy += x * y, ++nb;
    }
    const double slope = (nb * Sxy - Sx * Sy) / (nb * Sxx - Sx * Sx), icpt = (Sy - slope * Sx) / nb;
    swcalib::fit(H.data(), 200, &c);
    CHECK(c.status == 0 && c.fits == 1 && c.n_fit == 4400 && c.n_db == 4400, "closed form: status %d fits %d", c.status, c.fits);
    CHECK(near(c.c, slope, 1e-9) && near(c.a, icpt, 1e-9), "closed form: a %.12g (%.12g) c %.12g (%.12g)", c.a, icpt, c.c, slope);
    const sw_calib base = c;
    // counts in the clip column change no coefficient
    H[30 * kSBins + kSBins - 1] = 7;
    swcalib::fit(H.data(), 200, &c);
    CHECK(c.a == base.a && c.c == base.c && c.sigma == base.sigma && c.n_clipped == 7 && c.n_db == 4407 && c.status == 0, "clip column");
    // a planted outlier is trimmed and the fit returns to the clean one's
    H[30 * kSBins + kSBins - 1] = 0;
    H[30 * kSBins + 400] = 3;
    swcalib::fit(H.data(), 200, &c);
    CHECK(c.fits >= 2 && c.n_fit == 4400 && near(c.a, base.a, 1e-12) && near(c.c, base.c, 1e-12), "outlier: fits %d n_fit %lld", c.fits, (long long)c.n_fit);

    // ---- significance -----------------------------------------------------------
    swcalib::significance(base, 0, 300, &s);
    CHECK(s.evalue == 4400 && s.bits == 0, "zero score");
    swcalib::significance(base, 40, 0, &s);
    CHECK(s.evalue == 4400 && s.bits == 0, "empty subject");
    swcalib::significance(base, 500, 300, &s);  // far in the tail: E keeps its digits (expm1)
    CHECK(s.evalue > 0 && s.evalue < 1e-30 && s.bits > 100, "tail E %g bits %g", s.evalue, s.bits);
    const double t = 1.2825498301618641 * s.z + 0.5772156649015329;
    CHECK(near(s.evalue, 4400 * std::exp(-t), 1e-9), "tail E %g vs n e^-t %g", s.evalue, 4400 * std::exp(-t));
    swcalib::significance(base, 1, 300, &s);  // far below the line: E = n_db
    CHECK(near(s.evalue, 4400, 1e-6), "low E %g", s.evalue);

    if (g_fail) return 1;
    std::printf("calib_check ok\n");
    return 0;
}
