// sw_calib.cpp — the calibration's host half (sw_calib.h): the weighted
// regression of score on ln(length) over the device's count table, its
// trimming, and the extreme-value significance of a hit.  Doubles throughout;
// nothing here touches HIP.
#include "sw_calib.h"

#include <cmath>
#include <vector>

namespace swcalib {

namespace {
constexpr double kPiOverSqrt6 = 1.2825498301618640955;  // pi / sqrt(6)
constexpr double kEulerGamma = 0.57721566490153286061;
constexpr double kLn2 = 0.69314718055994530942;

struct Cell {
    int b, s;
    double x, w;
};
}  // namespace

double bin_abscissa(int b) {
    const int e = b >> 2, f = b & 3;
    return std::log(std::ldexp(1.0 + (f + 0.5) / 4.0, e));
}

void fit(const uint32_t* hist, int32_t qlen, sw_calib* out) {
    *out = sw_calib{};
    out->size = static_cast<int32_t>(sizeof(sw_calib));
    out->qlen = qlen;
    // the occupied cells below the clip column; the clip column only counts
    std::vector<Cell> cells;
    for (int b = 0; b < kLBins; ++b) {
        const double x = bin_abscissa(b);
        for (int s = 0; s < kSBins; ++s) {
            const uint32_t w = hist[b * kSBins + s];
            if (!w) continue;
            out->n_db += w;
            if (s == kSBins - 1)
                out->n_clipped += w;
            else
                cells.push_back(Cell{b, s, x, static_cast<double>(w)});
        }
    }
    if (out->n_clipped * 100 > out->n_db) out->status |= SW_CALIB_CLIPPED;

    std::vector<char> keep(cells.size(), 1), next(cells.size());
    int bins_kept = 0;
    bool degenerate = false;
    for (int round = 1; round <= kMaxFits; ++round) {
        // the kept set's weight, means and occupied length bins
        double W = 0, Sx = 0, Ss = 0;
        int64_t n = 0;
        bool occupied[kLBins] = {};
        for (size_t i = 0; i < cells.size(); ++i) {
            if (!keep[i]) continue;
            const Cell& c = cells[i];
            W += c.w;
            Sx += c.w * c.x;
            Ss += c.w * c.s;
            n += static_cast<int64_t>(c.w);
            occupied[c.b] = true;
        }
        bins_kept = 0;
        for (bool o : occupied) bins_kept += o;
        out->n_fit = n;
        const double ms = W > 0 ? Ss / W : 0.0;
        degenerate = true;
        out->a = ms;
        out->c = 0;
        out->sigma = 0;
        if (W < 3 || bins_kept < 2) break;
        const double mx = Sx / W;
        double Sxx = 0, Sxy = 0;
        for (size_t i = 0; i < cells.size(); ++i) {
            if (!keep[i]) continue;
            const Cell& c = cells[i];
            Sxx += c.w * (c.x - mx) * (c.x - mx);
            Sxy += c.w * (c.x - mx) * (c.s - ms);
        }
        if (!(Sxx > 0)) break;
        const double slope = Sxy / Sxx, icpt = ms - slope * mx;
        double rss = 0;
        for (size_t i = 0; i < cells.size(); ++i) {
            if (!keep[i]) continue;
            const Cell& c = cells[i];
            const double r = c.s - icpt - slope * c.x;
            rss += c.w * r * r;
        }
        const double sigma = std::sqrt(rss / (W - 2));
        if (!(sigma > 0)) break;
        degenerate = false;
        out->a = icpt;
        out->c = slope;
        out->sigma = sigma;
        out->fits = round;
        if (round == kMaxFits) break;
        // every cell is tested again under the latest fit: one that left may return
        bool same = true;
        for (size_t i = 0; i < cells.size(); ++i) {
            const Cell& c = cells[i];
            const double t = (c.s - icpt - slope * c.x) / sigma;
            next[i] = !(t > kTrim || t < -kTrim);
            same = same && next[i] == keep[i];
        }
        if (same) break;
        keep.swap(next);
    }
    if (degenerate) out->status |= SW_CALIB_DEGENERATE;
    if (bins_kept < 3 || out->n_fit < 500) out->status |= SW_CALIB_FEW;
}

void significance(const sw_calib& c, int32_t score, int32_t slen, sw_sig* out) {
    out->z = 0;
    out->evalue = static_cast<double>(c.n_db);
    out->bits = 0;
    if ((c.status & SW_CALIB_DEGENERATE) || !(c.sigma > 0) || slen <= 0 || score <= 0 || c.qlen <= 0) return;
    const double lnL = std::log(static_cast<double>(slen));
    const double z = (score - c.a - c.c * lnL) / c.sigma;
    const double t = kPiOverSqrt6 * z + kEulerGamma;
    out->z = z;
    out->evalue = static_cast<double>(c.n_db) * -std::expm1(-std::exp(-t));
    out->bits = (t + std::log(static_cast<double>(c.qlen) * static_cast<double>(slen))) / kLn2;
}

static bool degenerate(const sw_calib& c) { return (c.status & SW_CALIB_DEGENERATE) || !(c.sigma > 0); }

void rank_table(const sw_calib& c, int32_t max_len, int32_t* adj) {
    const bool flat = degenerate(c);
    adj[0] = 0;
    for (int64_t L = 1; L <= max_len; ++L) {  // (64-bit: max_len = INT32_MAX ends the loop)
        if (flat) {
            adj[L] = 0;
            continue;
        }
        const double v = static_cast<double>(kRankScale) * c.c * std::log(static_cast<double>(L));
        adj[L] = v >= 2147483647.0 ? INT32_MAX : v <= -2147483648.0 ? INT32_MIN : static_cast<int32_t>(std::llround(v));
    }
}

bool rank_min(const sw_calib& c, double max_evalue, int64_t* r_min) {
    if (!(max_evalue > 0)) return false;  // (NaN too)
    const double n_db = static_cast<double>(c.n_db);
    if (max_evalue >= n_db) {  // (+inf too)
        *r_min = kRankFloor;
        return true;
    }
    if (degenerate(c)) {  // every E-value is n_db
        *r_min = kRankNone;
        return true;
    }
    // E = n_db (1 - exp(-exp(-t))), t = (pi / sqrt 6) z + gamma, solved for z
    const double t = -std::log(-std::log1p(-max_evalue / n_db));
    const double z_min = (t - kEulerGamma) / kPiOverSqrt6;
    const double v = std::ceil(static_cast<double>(kRankScale) * (c.a + c.sigma * z_min));
    // (a real cutoff stays above the floor: a subject of score <= 0 has E = n_db)
    *r_min = !(v > static_cast<double>(kRankFloor)) ? kRankFloor + 1
             : v >= static_cast<double>(kRankNone)  ? kRankNone
                                                    : static_cast<int64_t>(v);
    return true;
}

}  // namespace swcalib
