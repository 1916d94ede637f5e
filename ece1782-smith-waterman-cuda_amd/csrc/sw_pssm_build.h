// sw_pssm_build.h — from integer profile tables to a position-specific scoring
// matrix (include/sw_amd.h "iterated profile search", step 3): pure host C++,
// no handle, no HIP.  The tables are sw_msa.hip's; the background frequencies
// are the Swiss-Prot composition the synthetic generator draws from
// (sw_synth_host.h), normalised.
#pragma once

#include <cstdint>

namespace swprofile {

constexpr int kCodes = 20;      // the counted residue codes 0..19
constexpr int kAlphabet = 25;   // columns of a PSSM row
constexpr int kMaxEntry = 100;  // entries are clamped to -100..100 (sw_pssm_create's range)

// p[20]: the normalised background.
void background(double* p);

// The positive root of sum_{a,b<20} p_a p_b exp(lambda s[a][b]) = 1 for a
// 25 x 25 matrix: bisection in doubles (hi doubles from 1 until f(hi) > 0, lo
// halves from hi until f(lo) < 0, then halving until the midpoint equals an
// end; the lower end is returned).  false: no root (the expected score is not
// negative, or no entry is positive).
bool matrix_lambda(const int8_t* matrix, double* lambda);

// rows_out[qlen][25] from cnt[qlen][20], wsum[qlen][20], the prior table and
// the matrix (pseudo in (0, 1000], checked by the caller).  false: the matrix
// has no lambda.  rows_out may alias prior_rows.
bool pssm_from_counts(const uint32_t* cnt, const uint64_t* wsum, int32_t qlen, const int8_t* prior_rows,
                      const int8_t* matrix, double pseudo, int8_t* rows_out);

}  // namespace swprofile
