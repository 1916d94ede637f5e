// sw_profile.hip — the query profiles built on the device: from the query
// codes and the scoring matrix carried in the kernel arguments
// (sw_build_profile), or from a position-specific scoring matrix resident in
// HBM (sw_build_profile_pssm, at the end).
//
// The reference builds nothing per query: its kernel reads the BLOSUM50 table
// and the query from __constant__ memory (SWSolver.cu:54-81, 296-299, 246),
// one lookup per cell.  Here every scan kernel reads a per-query profile
// (prof[stored code][row] = S[q_row][code], + the gap for the linear kernels;
// the database stores code c as kStored[c], sw_kernels.h), so a
// scan starts by building it.  Built on the host and copied, each scan paid
// an H2D copy on the DMA engine plus the compute queue's wait for it, ~30-40
// us between two scans (rocprofv3 trace of C2's 1/8 share, profiles/r03_trace/);
// a kernel on the scan's own queue costs a few microseconds and needs no copy:
// the query and the matrix travel inside the launch's kernel arguments.
#include "sw_kernels.h"

namespace swk {

// The first launch of a scan resets the rescue lists' counters and heads and
// the merged launch's work counter.
template <class A>
__device__ __forceinline__ void profile_reset(const A& a) {
    if (blockIdx.x == 0 && threadIdx.x < 10) {
        int32_t* p = a.reset[threadIdx.x];
        if (p) *p = threadIdx.x == 2 ? -1 : 0;
    }
}

// Entry (stored code c, query row i) = v in every image the scan asked for.
template <class A>
__device__ __forceinline__ void profile_store(const A& a, int c, int i, int v) {
    if (i < a.stride) {
        const size_t k = static_cast<size_t>(c) * a.stride + i;
        a.p8[k] = static_cast<int8_t>(v);
        if (a.p16) a.p16[k] = static_cast<int16_t>(v);
    }
    if (a.pin && i < a.qpad_intra) {
        // lane-slotted image of the int32 intra kernel: [chunk][code][lane][RIP]
        const int ch = i / (kLanes * a.ri), w = i % (kLanes * a.ri);
        const int t = w / a.ri, r = w % a.ri;
        int8_t* d = a.pin + ((static_cast<size_t>(ch) * kProfileRows + c) * kLanes + t) * a.rip;
        d[r] = static_cast<int8_t>(v);
        if (r == a.ri - 1)
            for (int p = a.ri; p < a.rip; ++p) d[p] = 0;
    }
}

// One thread per (code, row) entry of rows [row0, row1).
__global__ __launch_bounds__(256) void sw_build_profile(ProfileArgs a) {
    profile_reset(a);
    const int n = a.row1 - a.row0;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= kProfileRows * n) return;
    const int c = tid / n;  // the profile row: a STORED code (sw_kernels.h kStored)
    const int i = a.row0 + tid % n;
    const int v =
        (c >= kAlphabet || i >= a.qlen) ? a.bias : a.mat[kAlphabet * a.q[i - a.row0] + kCodeOf[c]] + a.bias;
    profile_store(a, c, i, v);
}

// The same images from a position-specific scoring matrix resident in HBM
// (sw_pssm_create): one thread per (code, row) entry of rows [0, rows), one
// launch for any query length.  The resident table is TRANSPOSED,
// pssm[code][ld] with ld >= qlen: consecutive threads are consecutive rows of
// one code, so a wave reads 64 consecutive bytes (row-major [qlen][25] would
// put them 25 bytes apart).
__global__ __launch_bounds__(256) void sw_build_profile_pssm(PssmProfileArgs a) {
    profile_reset(a);
    const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (tid >= static_cast<int64_t>(kProfileRows) * a.rows) return;
    const int c = static_cast<int>(tid / a.rows);  // a STORED code
    const int i = static_cast<int>(tid % a.rows);
    const int8_t* __restrict__ t = a.pssm;
    const int v = (c >= kAlphabet || i >= a.qlen) ? a.bias : t[static_cast<size_t>(kCodeOf[c]) * a.ld + i] + a.bias;
    profile_store(a, c, i, v);
}

hipError_t launch_build_profile(const ProfileArgs& a, hipStream_t s) {
    const int n = a.row1 - a.row0;
    if (n <= 0 || n > kProfQueryChunk) return hipErrorInvalidValue;
    const int threads = kProfileRows * n;
    hipLaunchKernelGGL(sw_build_profile, dim3((threads + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_build_profile_pssm(const PssmProfileArgs& a, hipStream_t s) {
    if (a.rows <= 0 || !a.pssm || a.ld < a.qlen) return hipErrorInvalidValue;
    const int64_t threads = static_cast<int64_t>(kProfileRows) * a.rows;
    hipLaunchKernelGGL(sw_build_profile_pssm, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace swk
