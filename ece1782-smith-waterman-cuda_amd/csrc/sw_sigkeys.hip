// sw_sigkeys.hip — ranking by E-value (include/sw_amd.h "ranking by
// E-value"): the device pass between a scan's fit and its ranking.
//
// sw_sig_keys: 256-thread workgroups over 1,024 consecutive subjects, four per
// thread a workgroup's width apart (a wave reads and writes consecutive
// subjects).  A thread reads its subject's result id, length and score and
// the length's adjustment adj[min(L, max_len)] (a table of a few hundred KB at
// most, resident in L2), forms the rank value and its key
// (swcalib::rank_value, rank_key: integer only, the host's functions), and
// writes the key, or INT64_MIN below r_min.  The subjects that pass are
// counted exactly: a ballot and a popcount per wave and round, the four waves'
// sums through LDS, then one vector atomic add per workgroup with a passing
// subject into a uint32 in device memory.  (One add per wave of one subject
// per thread was measured first: with no cutoff every wave of C2's 570,000
// subjects adds, 8,906 atomics on one address, and the kernel took 104 us;
// under a cutoff few subjects pass and it took 3.7 us.)  Only score slots a
// subject maps to are read.
//
// sw_sig_gather: the rows of the selected keys for the form that has no hit
// table (PSSM scans): {id, score, subject length, 0}.  A key carries the
// result id, and the lengths are indexed by SUBJECT, so the row of a selected
// key is written by its subject's thread: one thread per subject again, which
// reads its own key back (keys[i], what sw_sig_keys wrote), leaves unless the
// key is at or above the last selected one, and finds its row by a binary
// search of the k selected keys (sorted, best first).
#include <hip/hip_runtime.h>

#include "sw_calib.h"
#include "sw_kernels.h"

namespace swk {

constexpr int kSigThreads = 256;
constexpr int kSigPer = 4;                           // subjects per thread (sw_sig_keys)
constexpr int kSigChunk = kSigThreads * kSigPer;     // subjects per workgroup
constexpr int64_t kSigPad = INT64_MIN;

__global__ __launch_bounds__(kSigThreads) void sw_sig_keys(const int32_t* __restrict__ scores,
                                                          const int32_t* __restrict__ rid,
                                                          const int32_t* __restrict__ slen,
                                                          const int32_t* __restrict__ adj, int32_t max_len,
                                                          int64_t r_min, int64_t n, int64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_sum[kSigThreads / 64];
    const int t = threadIdx.x;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kSigChunk;
    uint32_t passed = 0;  // wave-uniform: this wave's passing subjects
#pragma unroll
    for (int j = 0; j < kSigPer; ++j) {
        const int64_t i = base + j * kSigThreads + t;
        bool pass = false;
        if (i < n) {
            const int32_t id = rid ? rid[i] : static_cast<int32_t>(i);
            const int32_t L = slen[i];
            const int32_t a = adj[L < 0 ? 0 : L > max_len ? max_len : L];
            const int64_t r = swcalib::rank_value(scores[id], L, a);
            pass = r >= r_min;
            keys[i] = pass ? swcalib::rank_key(r, id) : kSigPad;
        }
        passed += static_cast<uint32_t>(__popcll(__ballot(pass)));
    }
    if ((t & 63) == 0) wave_sum[t >> 6] = passed;
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kSigThreads / 64; ++w) total += wave_sum[w];
        if (total) atomicAdd(count, total);
    }
}

__global__ __launch_bounds__(kSigThreads) void sw_sig_gather(const int32_t* __restrict__ scores,
                                                            const int32_t* __restrict__ rid,
                                                            const int32_t* __restrict__ slen,
                                                            const int64_t* __restrict__ keys, int64_t n,
                                                            const int64_t* __restrict__ sel, int32_t k,
                                                            int32_t* __restrict__ rows) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSigThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t key = keys[i];
    if (key == kSigPad || key < sel[k - 1]) return;  // (sel[k - 1] is INT64_MIN when fewer than k passed)
    // sel is strictly descending over its non-absent keys: the first p with sel[p] <= key
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sel[mid] <= key) hi = mid;
        else lo = mid + 1;
    }
    if (sel[lo] != key) return;
    const int32_t id = rid ? rid[i] : static_cast<int32_t>(i);
    int32_t* const o = rows + 4 * static_cast<int64_t>(lo);
    o[0] = id;
    o[1] = scores[id];
    o[2] = slen[i];
    o[3] = 0;
}

hipError_t launch_sig_keys(const int32_t* scores, const int32_t* rid, const int32_t* slen, const int32_t* adj,
                           int32_t max_len, int64_t r_min, int64_t n, int64_t* keys, uint32_t* count, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t grid = (n + kSigChunk - 1) / kSigChunk;
    hipLaunchKernelGGL(sw_sig_keys, dim3(static_cast<unsigned>(grid)), dim3(kSigThreads), 0, s, scores, rid, slen,
                       adj, max_len, r_min, n, keys, count);
    return hipGetLastError();
}

hipError_t launch_sig_gather(const int32_t* scores, const int32_t* rid, const int32_t* slen, const int64_t* keys,
                             int64_t n, const int64_t* sel, int32_t k, int32_t* rows, hipStream_t s) {
    if (n <= 0 || k <= 0) return hipSuccess;
    const int64_t grid = (n + kSigThreads - 1) / kSigThreads;
    hipLaunchKernelGGL(sw_sig_gather, dim3(static_cast<unsigned>(grid)), dim3(kSigThreads), 0, s, scores, rid, slen,
                       keys, n, sel, k, rows);
    return hipGetLastError();
}

}  // namespace swk
