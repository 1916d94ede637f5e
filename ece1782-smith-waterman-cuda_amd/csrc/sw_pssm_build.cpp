// sw_pssm_build.cpp — sw_pssm_build.h's host arithmetic.
#include "sw_pssm_build.h"

#include <algorithm>
#include <cmath>

#include "sw_synth_host.h"

namespace swprofile {

void background(double* p) {
    double sum = 0;
    for (double f : swk::kSwissProtFreq) sum += f;
    for (int a = 0; a < kCodes; ++a) p[a] = swk::kSwissProtFreq[a] / sum;
}

namespace {

// f(lambda) = sum p_a p_b exp(lambda s[a][b]) - 1
double lambda_f(const int8_t* m, const double* p, double lambda) {
    double s = 0;
    for (int a = 0; a < kCodes; ++a)
        for (int b = 0; b < kCodes; ++b) s += p[a] * p[b] * std::exp(lambda * m[kAlphabet * a + b]);
    return s - 1.0;
}

}  // namespace

bool matrix_lambda(const int8_t* m, double* lambda) {
    double p[kCodes];
    background(p);
    double mean = 0;
    bool positive = false;
    for (int a = 0; a < kCodes; ++a)
        for (int b = 0; b < kCodes; ++b) {
            mean += p[a] * p[b] * m[kAlphabet * a + b];
            positive = positive || m[kAlphabet * a + b] > 0;
        }
    if (!(mean < 0) || !positive) return false;
    // entries are int8, so hi stays far below the doubles' range: a positive
    // entry s makes f(hi) > 0 once p_a p_b exp(hi s) > 1, hi <= 16
    double hi = 1.0;
    while (!(lambda_f(m, p, hi) > 0)) hi *= 2;
    double lo = hi;
    // f < 0 just right of 0 (f(0) = 0, f'(0) = mean < 0); a dip the doubles cannot see is no root
    while (!(lambda_f(m, p, lo) < 0))
        if ((lo *= 0.5) < 1e-12) return false;
    for (;;) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        if (lambda_f(m, p, mid) > 0) hi = mid;
        else lo = mid;
    }
    *lambda = lo;
    return true;
}

bool pssm_from_counts(const uint32_t* cnt, const uint64_t* wsum, int32_t qlen, const int8_t* prior, const int8_t* m,
                      double pseudo, int8_t* out) {
    double lambda = 0, p[kCodes], e[kCodes][kCodes];
    if (!matrix_lambda(m, &lambda)) return false;
    background(p);
    for (int b = 0; b < kCodes; ++b)
        for (int a = 0; a < kCodes; ++a) e[b][a] = std::exp(lambda * m[kAlphabet * b + a]);  // row: the query side
    for (int32_t i = 0; i < qlen; ++i) {
        const uint32_t* c = cnt + static_cast<int64_t>(i) * kCodes;
        const uint64_t* w = wsum + static_cast<int64_t>(i) * kCodes;
        const int8_t* pr = prior + static_cast<int64_t>(i) * kAlphabet;
        int8_t* o = out + static_cast<int64_t>(i) * kAlphabet;
        uint64_t T = 0;
        int k = 0;
        for (int a = 0; a < kCodes; ++a) {
            T += w[a];
            k += c[a] != 0;
        }
        if (T == 0) {  // nothing observed: the prior row
            for (int a = 0; a < kAlphabet; ++a) o[a] = pr[a];
            continue;
        }
        double f[kCodes];
        for (int a = 0; a < kCodes; ++a) f[a] = static_cast<double>(w[a]) / static_cast<double>(T);
        const double alpha = std::max(k, 1) - 1, beta = pseudo;
        int8_t row[kAlphabet];
        for (int a = 0; a < kCodes; ++a) {
            double g = 0;
            for (int b = 0; b < kCodes; ++b) g += f[b] * e[b][a];
            g *= p[a];
            const double Q = (alpha * f[a] + beta * g) / (alpha + beta);
            const long long v = std::llround(std::log(Q / p[a]) / lambda);
            row[a] = static_cast<int8_t>(std::min<long long>(kMaxEntry, std::max<long long>(-kMaxEntry, v)));
        }
        for (int a = kCodes; a < kAlphabet; ++a) row[a] = pr[a];
        for (int a = 0; a < kAlphabet; ++a) o[a] = row[a];
    }
    return true;
}

}  // namespace swprofile
