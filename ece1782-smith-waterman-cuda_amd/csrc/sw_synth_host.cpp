// sw_synth_host.cpp — the synthetic generator's tables and host restatement
// (sw_synth_host.h).
#include "sw_synth_host.h"

#include <algorithm>
#include <cmath>

#include "sw_kernels.h"
#include "sw_synth_hash.h"

namespace swk {

namespace {

constexpr uint64_t kLenSalt = 0x4C454E475448ull;  // "LENGTH"

// Acklam's rational approximation of the standard normal quantile.
double norm_quantile(double p) {
    static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                                1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                                6.680131188771972e+01, -1.328068155288572e+01};
    static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                                -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                                3.754408661907416e+00};
    const double pl = 0.02425;
    if (p < pl) {
        const double q = std::sqrt(-2 * std::log(p));
        return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
               ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
    }
    if (p > 1 - pl) {
        const double q = std::sqrt(-2 * std::log(1 - p));
        return -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
               ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
    }
    const double q = p - 0.5, r = q * q;
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
           (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1);
}

}  // namespace

SynthTables::SynthTables() {
    for (int k = 0; k < 4096; ++k) {
        const double z = norm_quantile((k + 0.5) / 4096.0);
        const double L = std::nearbyint(std::exp(std::log(290.0) + 0.657 * z));
        len[k] = static_cast<int32_t>(std::min(35213.0, std::max(5.0, L)));
    }
    double sum = 0, acc = 0;
    for (double f : kSwissProtFreq) sum += f;
    int64_t edges[20];
    for (int c = 0; c < 20; ++c) {
        acc += kSwissProtFreq[c] / sum;
        edges[c] = static_cast<int64_t>(std::nearbyint(acc * 65536.0));
    }
    edges[19] = 65536;
    int c = 0;
    for (int v = 0; v < 65536; ++v) {
        while (c < 19 && edges[c] <= v) ++c;
        lut[v] = static_cast<uint8_t>(c);
        lut_stored[v] = kStored[c];
    }
}

const SynthTables& synth_tables() {
    static const SynthTables t;
    return t;
}

int32_t synth_length(uint64_t seed, uint64_t gid) {
    return synth_tables().len[syn_hash(seed, gid, kLenSalt) >> 52];
}

void synth_residues(uint64_t seed, uint64_t gid, int64_t L, uint8_t* out) {
    const uint8_t* lut = synth_tables().lut;
    for (int64_t j = 0; j < L; j += 4) {
        const uint64_t h = syn_hash(seed, gid, static_cast<uint64_t>(j >> 2));
        for (int e = 0; e < 4 && j + e < L; ++e) out[j + e] = lut[(h >> (16 * e)) & 0xffffu];
    }
}

}  // namespace swk
