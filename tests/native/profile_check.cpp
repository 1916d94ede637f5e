// profile_check.cpp — stand-alone program over the profile builder's host
// arithmetic (csrc/sw_pssm_build.cpp): built with -fsanitize=address,undefined
// by tests/test_profile_cpu.py and run as a program.  Prints "profile_check ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sw_pssm_build.h"

using namespace swprofile;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

// +match on the diagonal, -mismatch elsewhere (all 25 codes)
static std::vector<int8_t> diag_matrix(int match, int mismatch) {
    std::vector<int8_t> m(625);
    for (int a = 0; a < 25; ++a)
        for (int b = 0; b < 25; ++b) m[25 * a + b] = static_cast<int8_t>(a == b ? match : -mismatch);
    return m;
}

int main() {
    double p[kCodes], S = 0, sum = 0;
    background(p);
    for (int a = 0; a < kCodes; ++a) sum += p[a], S += p[a] * p[a];
    CHECK(std::fabs(sum - 1.0) < 1e-14);

    // lambda of +3 / -3 in closed form: S x + (1 - S) / x = 1 with x = exp(3 lambda) -> x = (1 - S) / S
    const std::vector<int8_t> id3 = diag_matrix(3, 3);
    double lam = 0;
    CHECK(matrix_lambda(id3.data(), &lam));
    CHECK(std::fabs(lam - std::log((1 - S) / S) / 3) < 1e-12 * lam);
    // no root: all positive; a non-negative expectation; no positive entry
    double unused = -1;
    CHECK(!matrix_lambda(std::vector<int8_t>(625, 2).data(), &unused));
    CHECK(!matrix_lambda(diag_matrix(100, 1).data(), &unused));
    CHECK(!matrix_lambda(std::vector<int8_t>(625, -1).data(), &unused));
    CHECK(unused == -1);
    // the extremes of int8 still bracket
    CHECK(matrix_lambda(diag_matrix(127, 128).data(), &lam) && lam > 0);
    CHECK(matrix_lambda(diag_matrix(1, 128).data(), &lam) && lam > 0);

    // tables of 4 positions: one observed residue, nothing observed, two residues, all twenty
    const int qlen = 4;
    std::vector<uint32_t> cnt(qlen * kCodes, 0);
    std::vector<uint64_t> wsum(qlen * kCodes, 0);
    std::vector<int8_t> prior(qlen * kAlphabet), rows(qlen * kAlphabet, 0);
    for (int i = 0; i < qlen * kAlphabet; ++i) prior[i] = static_cast<int8_t>(i % 7 - 3);
    cnt[0 * kCodes + 5] = 3, wsum[0 * kCodes + 5] = 123456789;
    cnt[2 * kCodes + 1] = 1, wsum[2 * kCodes + 1] = 1ull << 42;
    cnt[2 * kCodes + 9] = 4000, wsum[2 * kCodes + 9] = 7;
    for (int a = 0; a < kCodes; ++a) cnt[3 * kCodes + a] = 1 + a, wsum[3 * kCodes + a] = (1ull << 30) / (a + 1);
    CHECK(pssm_from_counts(cnt.data(), wsum.data(), qlen, prior.data(), id3.data(), 10.0, rows.data()));
    for (int a = 0; a < kCodes; ++a) CHECK(rows[a] == id3[25 * 5 + a]);  // alpha = 0: the matrix's row
    for (int a = kCodes; a < kAlphabet; ++a) CHECK(rows[a] == prior[a]);
    CHECK(std::memcmp(&rows[kAlphabet], &prior[kAlphabet], kAlphabet) == 0);  // T = 0: the prior row
    CHECK(rows[2 * kAlphabet + 1] > 0 && rows[2 * kAlphabet + 9] <= rows[2 * kAlphabet + 1]);
    for (int i = 0; i < qlen * kAlphabet; ++i) CHECK(rows[i] >= -kMaxEntry && rows[i] <= kMaxEntry);
    // in place (rows_out aliases the prior), and the pseudocount's ends
    std::vector<int8_t> inplace = prior;
    CHECK(pssm_from_counts(cnt.data(), wsum.data(), qlen, inplace.data(), id3.data(), 10.0, inplace.data()));
    CHECK(inplace == rows);
    CHECK(pssm_from_counts(cnt.data(), wsum.data(), qlen, prior.data(), id3.data(), 1e-300, rows.data()));
    CHECK(pssm_from_counts(cnt.data(), wsum.data(), qlen, prior.data(), id3.data(), 1000.0, rows.data()));
    // entries clamp: a steep matrix with one observed residue
    const std::vector<int8_t> steep = diag_matrix(127, 128);
    CHECK(pssm_from_counts(cnt.data(), wsum.data(), 1, prior.data(), steep.data(), 10.0, rows.data()));
    CHECK(rows[5] == kMaxEntry && rows[0] == -kMaxEntry);
    // no position; a matrix without lambda
    CHECK(pssm_from_counts(nullptr, nullptr, 0, nullptr, id3.data(), 10.0, nullptr));
    CHECK(!pssm_from_counts(cnt.data(), wsum.data(), qlen, prior.data(), std::vector<int8_t>(625, 2).data(), 10.0, rows.data()));

    if (failures) return 1;
    std::printf("profile_check ok\n");
    return 0;
}
