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

}  // namespace swcalib

#endif  // SW_CALIB_H
