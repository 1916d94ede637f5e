// sw_calib.h — per-scan calibration of E-values and bit scores (pure C++: no
// HIP include; tests/native/calib_check.cpp compiles sw_calib.cpp alone).
//
// The library takes any 625-entry matrix, any gap pair and a PSSM, so a table
// of Karlin-Altschul constants cannot serve it.  What fits every scoring is
// SSEARCH's way: calibrate on the scan's own scores.  A device pass
// (sw_calib.hip) counts every subject's score into a length-bin x score
// table; the host regresses score on ln(length) over that table, trims the
// related sequences, and turns a hit's z-score into an extreme-value E-value.
// The definitions (bin, table, fit, status, significance) are include/
// sw_amd.h's; this file is their one implementation, host and device.
#ifndef SW_CALIB_H
#define SW_CALIB_H

#include <cstdint>

#include "sw_amd.h"

#if defined(__HIPCC__)
#define SW_CALIB_HD __host__ __device__
#else
#define SW_CALIB_HD
#endif

namespace swcalib {

constexpr int kLBins = SW_CALIB_LBINS;  // length bins (rows)
constexpr int kSBins = SW_CALIB_SBINS;  // score columns; the last one clips
constexpr int kCells = kLBins * kSBins;
constexpr int kMaxFits = 8;
constexpr double kTrim = 5.0;  // cells with |r / sigma| above this leave the fit

// Length bin of a subject of length L >= 1: four bins per octave, from L's
// leading bit e and the two bits below it (integer only: the device and the
// host agree by construction).  L < 2^31 gives a bin < 124.
SW_CALIB_HD inline int length_bin(uint32_t L) {
    const int e = 31 - __builtin_clz(L);
    const uint32_t f = e >= 2 ? (L >> (e - 2)) & 3u : (L << (2 - e)) & 3u;
    return 4 * e + static_cast<int>(f);
}

// The bin's abscissa: ln of the middle of its length range.
double bin_abscissa(int b);

// Score column of a score: [0, 510] as is, everything above in the clip column.
SW_CALIB_HD inline int score_bin(int32_t s) { return s < 0 ? 0 : s > kSBins - 1 ? kSBins - 1 : s; }

// sw_calib_fit / sw_calib_sig (argument checks are the caller's).
void fit(const uint32_t* hist, int32_t qlen, sw_calib* out);
void significance(const sw_calib& c, int32_t score, int32_t slen, sw_sig* out);

// ---- ranking by E-value (include/sw_amd.h "ranking by E-value") --------------
// The rank value and its key, integer only: the host, the device pass
// (sw_sigkeys.hip) and the tests' restatement agree bit for bit.
constexpr int64_t kRankScale = SW_RANK_SCALE;
constexpr int64_t kRankFloor = SW_RANK_FLOOR;
constexpr int64_t kRankNone = SW_RANK_NONE;
constexpr int64_t kRankCeil = kRankNone - 1;       // 2^32 - 1
constexpr int32_t kRankMaxScore = (1 << 20) - 1;

// r(s, L) given adj = adj[min(L, max_len)].
SW_CALIB_HD inline int64_t rank_value(int32_t s, int32_t L, int32_t adj) {
    if (s <= 0 || L <= 0) return kRankFloor;
    const int64_t r = static_cast<int64_t>(s > kRankMaxScore ? kRankMaxScore : s) * kRankScale - adj;
    return r < kRankFloor ? kRankFloor : r > kRankCeil ? kRankCeil : r;
}
// r descending, then id ascending (0 <= id < 2^31); always above INT64_MIN.
SW_CALIB_HD inline int64_t rank_key(int64_t r, int32_t id) {
    return r * (int64_t{1} << 31) + ((int64_t{1} << 31) - 1 - id);
}
SW_CALIB_HD inline int32_t rank_key_id(int64_t key) {
    return static_cast<int32_t>((int64_t{1} << 31) - 1 - (key & ((int64_t{1} << 31) - 1)));
}

// sw_sig_rank_table / sw_sig_rank_min (argument checks are the caller's but
// max_evalue's: false for max_evalue <= 0 or NaN).
void rank_table(const sw_calib& c, int32_t max_len, int32_t* adj);
bool rank_min(const sw_calib& c, double max_evalue, int64_t* r_min);

}  // namespace swcalib

#endif  // SW_CALIB_H
