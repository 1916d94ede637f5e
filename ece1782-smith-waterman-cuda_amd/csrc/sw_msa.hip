// sw_msa.hip — the integer profile tables of a set of query-anchored alignment
// rows (include/sw_amd.h "iterated profile search"; the rows are what
// sw_align.hip's walk back writes through AlignArgs::msa, or a caller's).
//
// rows[nrows][qlen] bytes, row-major; only the codes 0..19 are counted (the
// ambiguity codes 20..24, kMsaGap and kMsaNone never are).  Three launches:
//
//   msa_col_counts   cnt[i][a]  = rows r with rows[r][i] == a
//                    term[i][a] = floor(2^30 / (k_i cnt[i][a])), k_i the codes
//                                 present in column i (Henikoff position-based
//                                 weights in fixed point); 0 where cnt is 0
//   msa_row_weights  weight[r]  = floor(sum_i term[i][rows[r][i]] / cov_r) over
//                                 the cov_r columns where row r holds a counted
//                                 code; 0 when cov_r is 0
//   msa_col_wsums    wsum[i][a] = sum of weight[r] over rows with rows[r][i] == a
//
// Everything is an integer, so the sums' order does not matter: host, device
// and tests agree bit for bit.  No float and no atomics anywhere.
//
// The two column kernels share a shape: a workgroup owns kMsaTile = 64
// consecutive columns, lane = column, so a wave reads 64 consecutive bytes of
// a row; its kMsaWaves waves take the rows r = wave (mod kMsaWaves).  Every
// thread keeps its 20 counters in LDS, laid out [wave][code][lane]: lane l
// only ever touches word l of a 64-word row, so an access hits 64 distinct
// banks' worth of consecutive words whatever the codes are (no conflicts
// beyond the 64-bit form's two passes), and no other thread writes them (no
// atomics).  After a barrier the waves' partial tables are summed, wave w
// folding the codes a = w (mod kMsaWaves).  A thread loads kMsaBatch rows'
// bytes before it counts them, so that the loads' latencies overlap.
// The row kernel is one wave per row: lanes stride the columns, the two sums
// are reduced across the wave in uint64 by shuffles.
#include "sw_kernels.h"

namespace swk {

namespace {

constexpr int kMsaThreads = kMsaTile * kMsaWaves;
constexpr uint32_t kProfileOne = 1u << 30;
// rows a thread loads before it counts them: the loads are independent, the
// LDS updates are not, and a thread's rows are about a thousand at most
constexpr int kMsaBatch = 8;

__global__ __launch_bounds__(kMsaThreads) void msa_col_counts(MsaArgs a) {
    __shared__ uint32_t c[kMsaWaves][kMsaCodes][kMsaTile];
    __shared__ uint32_t kcol[kMsaTile];
    const int lane = threadIdx.x % kMsaTile, w = threadIdx.x / kMsaTile;
    const int col = blockIdx.x * kMsaTile + lane;
    const bool live = col < a.qlen;
    for (int x = 0; x < kMsaCodes; ++x) c[w][x][lane] = 0;
    if (live) {
        const uint8_t* __restrict__ p = a.rows + col;
        for (int r0 = w; r0 < a.nrows; r0 += kMsaWaves * kMsaBatch) {
            uint32_t v[kMsaBatch];
#pragma unroll
            for (int u = 0; u < kMsaBatch; ++u) {
                const int r = r0 + u * kMsaWaves;
                v[u] = r < a.nrows ? p[static_cast<int64_t>(r) * a.qlen] : kMsaNone;
            }
#pragma unroll
            for (int u = 0; u < kMsaBatch; ++u)
                if (v[u] < kMsaCodes) ++c[w][v[u]][lane];
        }
    }
    __syncthreads();
    // fold the waves' tables into wave 0's, wave w taking the codes x = w (mod kMsaWaves)
    for (int x = w; x < kMsaCodes; x += kMsaWaves) {
        uint32_t t = 0;
        for (int u = 0; u < kMsaWaves; ++u) t += c[u][x][lane];
        c[0][x][lane] = t;  // (wave 0's word [x][lane] is read by this thread alone)
    }
    __syncthreads();
    if (w == 0) {
        uint32_t k = 0;
        for (int x = 0; x < kMsaCodes; ++x) k += c[0][x][lane] != 0;
        kcol[lane] = k;
    }
    __syncthreads();
    if (!live) return;
    const uint32_t k = kcol[lane];
    for (int x = w; x < kMsaCodes; x += kMsaWaves) {
        const uint32_t n = c[0][x][lane];
        const int64_t o = static_cast<int64_t>(col) * kMsaCodes + x;
        a.cnt[o] = n;
        a.term[o] = n ? kProfileOne / (k * n) : 0;
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int d = kLanes / 2; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), d, kLanes);
        const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), d, kLanes);
        v += (static_cast<uint64_t>(hi) << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(kMsaThreads) void msa_row_weights(MsaArgs a) {
    const int lane = threadIdx.x % kLanes;
    const int r = blockIdx.x * (kMsaThreads / kLanes) + threadIdx.x / kLanes;
    if (r >= a.nrows) return;  // (whole waves: no barrier follows)
    const uint8_t* __restrict__ p = a.rows + static_cast<int64_t>(r) * a.qlen;
    uint64_t u = 0, cov = 0;
    for (int i = lane; i < a.qlen; i += kLanes) {
        const uint32_t v = p[i];
        if (v < kMsaCodes) {
            u += a.term[static_cast<int64_t>(i) * kMsaCodes + v];
            ++cov;
        }
    }
    u = wave_sum(u);
    cov = wave_sum(cov);
    if (lane == 0) a.weight[r] = cov ? u / cov : 0;
}

__global__ __launch_bounds__(kMsaThreads) void msa_col_wsums(MsaArgs a) {
    __shared__ uint64_t c[kMsaWaves][kMsaCodes][kMsaTile];
    const int lane = threadIdx.x % kMsaTile, w = threadIdx.x / kMsaTile;
    const int col = blockIdx.x * kMsaTile + lane;
    const bool live = col < a.qlen;
    for (int x = 0; x < kMsaCodes; ++x) c[w][x][lane] = 0;
    if (live) {
        const uint8_t* __restrict__ p = a.rows + col;
        for (int r0 = w; r0 < a.nrows; r0 += kMsaWaves * kMsaBatch) {
            uint32_t v[kMsaBatch];
            uint64_t wt[kMsaBatch];
#pragma unroll
            for (int u = 0; u < kMsaBatch; ++u) {
                const int r = r0 + u * kMsaWaves;
                v[u] = r < a.nrows ? p[static_cast<int64_t>(r) * a.qlen] : kMsaNone;
                wt[u] = r < a.nrows ? a.weight[r] : 0;
            }
#pragma unroll
            for (int u = 0; u < kMsaBatch; ++u)
                if (v[u] < kMsaCodes) c[w][v[u]][lane] += wt[u];
        }
    }
    __syncthreads();
    if (!live) return;
    for (int x = w; x < kMsaCodes; x += kMsaWaves) {
        uint64_t t = 0;
        for (int u = 0; u < kMsaWaves; ++u) t += c[u][x][lane];
        a.wsum[static_cast<int64_t>(col) * kMsaCodes + x] = t;
    }
}

}  // namespace

hipError_t launch_msa_tables(const MsaArgs& a, hipStream_t s) {
    if (a.nrows <= 0 || a.qlen <= 0 || !a.rows || !a.cnt || !a.term || !a.weight || !a.wsum)
        return hipErrorInvalidValue;
    const unsigned tiles = static_cast<unsigned>((a.qlen + kMsaTile - 1) / kMsaTile);
    const unsigned rowblocks = static_cast<unsigned>((a.nrows + kMsaThreads / kLanes - 1) / (kMsaThreads / kLanes));
    hipLaunchKernelGGL(msa_col_counts, dim3(tiles), dim3(kMsaThreads), 0, s, a);
    hipLaunchKernelGGL(msa_row_weights, dim3(rowblocks), dim3(kMsaThreads), 0, s, a);
    hipLaunchKernelGGL(msa_col_wsums, dim3(tiles), dim3(kMsaThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace swk
