// sw_calib.hip — the calibration's device pass (sw_calib.h): one count per
// subject into the length-bin x score table uint32 hist[128][512].
//
// Per subject: result id (skipped when the ids are 0..n-1 in order), score,
// length, one count at [length_bin(L)][clamp(score, 0, 511)]; a subject of
// length 0 is not counted.  Integer only: the table is exact.
//
// Shape.  The scores of unrelated sequences crowd a few dozen columns of a
// few rows, so counting in HBM directly would put most of a database's
// atomics on a handful of addresses.  A workgroup instead owns a contiguous
// range of kCalibChunk subjects and keeps a WINDOW of kCalibRows table rows as
// LDS counters, starting at the lowest bin its range holds (four bins per
// octave: 32 rows span lengths 256:1, e.g. 10 .. 2,560); the rare subject
// whose bin lies above the window adds to HBM directly.  At the end the
// workgroup adds its non-zero counters to the table: one vector atomic per
// occupied cell and workgroup.  A range in length order (a loaded .swdb file)
// touches one or two rows; any order is exact.
#include <hip/hip_runtime.h>

#include "sw_calib.h"
#include "sw_kernels.h"

namespace swk {

constexpr int kCalibThreads = 256;
constexpr int kCalibPer = 16;                           // subjects per thread
constexpr int kCalibChunk = kCalibThreads * kCalibPer;  // subjects per workgroup
constexpr int kCalibRows = 32;                          // table rows held in LDS (64 KiB)

__global__ __launch_bounds__(kCalibThreads) void sw_score_hist(const int32_t* __restrict__ scores,
                                                              const int32_t* __restrict__ rid,
                                                              const int32_t* __restrict__ slen, int64_t n,
                                                              uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[kCalibRows * swcalib::kSBins];
    __shared__ int row0;
    const int t = threadIdx.x;
    const int64_t start = static_cast<int64_t>(blockIdx.x) * kCalibChunk;
    const int m = static_cast<int>(min(static_cast<int64_t>(kCalibChunk), n - start));  // subjects of this range
    if (t == 0) row0 = swcalib::kLBins - kCalibRows;  // the highest window that fits the table
    for (int i = t; i < kCalibRows * swcalib::kSBins; i += kCalibThreads) cnt[i] = 0;
    int bin[kCalibPer];
    int lo = swcalib::kLBins;
#pragma unroll
    for (int j = 0; j < kCalibPer; ++j) {
        const int i = j * kCalibThreads + t;
        const int32_t L = i < m ? slen[start + i] : 0;
        bin[j] = L > 0 ? swcalib::length_bin(static_cast<uint32_t>(L)) : -1;
        if (L > 0) lo = min(lo, bin[j]);
    }
    __syncthreads();
    if (lo < swcalib::kLBins - kCalibRows) atomicMin(&row0, lo);
    __syncthreads();
    const int base = row0;
#pragma unroll
    for (int j = 0; j < kCalibPer; ++j) {
        if (bin[j] < 0) continue;
        const int64_t g = start + j * kCalibThreads + t;
        const int col = swcalib::score_bin(scores[rid ? rid[g] : g]);
        const int row = bin[j] - base;
        if (row < kCalibRows)
            atomicAdd(&cnt[row * swcalib::kSBins + col], 1u);
        else
            atomicAdd(&hist[bin[j] * swcalib::kSBins + col], 1u);
    }
    __syncthreads();
    for (int i = t; i < kCalibRows * swcalib::kSBins; i += kCalibThreads)
        if (const uint32_t c = cnt[i]) atomicAdd(&hist[base * swcalib::kSBins + i], c);
}

hipError_t launch_score_hist(const int32_t* scores, const int32_t* rid, const int32_t* slen, int64_t n,
                             uint32_t* hist, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t grid = (n + kCalibChunk - 1) / kCalibChunk;
    hipLaunchKernelGGL(sw_score_hist, dim3(static_cast<unsigned>(grid)), dim3(kCalibThreads), 0, s, scores, rid,
                       slen, n, hist);
    return hipGetLastError();
}

}  // namespace swk
