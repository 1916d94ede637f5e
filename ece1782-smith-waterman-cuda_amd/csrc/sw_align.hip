// sw_align.hip — GPU traceback of chosen hits.
//
// The reference prints alignments only from its CPU program: cpu.cpp:47-70
// fills H with a direction per cell (left, then up, then diagonal, each
// taken only on a STRICT improvement over the running value that starts at
// 0), keeps the first strict maximum in row-major order, and walks back
// while the cell is non-zero (cpu.cpp:76-108).  sw_align_linear reproduces
// those rules exactly for any substitution matrix and a linear gap, one hit
// per workgroup; sw_align_affine extends them to affine gaps (below):
//
//  * fill: an anti-diagonal sweep (cells i + j = d are independent); the
//    three most recent diagonals of H live in a per-hit global scratch
//    (3 x (qlen+1) int32, so query length is unbounded), the direction of
//    every cell is stored as one byte in a diagonal-major array T[d][i]
//    (consecutive threads write consecutive bytes);
//  * best cell: per-thread (value, i, j) maxima with the row-major tie rule,
//    reduced across the workgroup;
//  * walk back: one thread follows T from the best cell, writing the ops
//    (M aligned pair, I query residue vs gap, D subject residue vs gap).
//
// Cost is O(|q| |s|) per hit — meant for the top hits of a scan, not the
// database.
//
// Both sweeps are templates over a score functor for the diagonal term: a
// residue sequence against the matrix (MatScore), or a position-specific
// scoring matrix (PssmScore, sw_align_pssm), whose term is pssm[i-1][s[j-1]]
// read from the resident table.  Tie rules, scratch layout and the walk back
// are the same code.
#include "sw_kernels.h"

namespace swk {

constexpr int kAlignThreads = 256;

struct Best {
    int h, i, j;
};

// (h, i, j) ordering of cpu.cpp's scan: larger h wins; on equal h the cell
// met first in row-major order (smaller i, then smaller j); h == 0 never
// replaces the initial (0, 0, 0).
__device__ __forceinline__ bool better(const Best& x, const Best& y) {
    if (x.h != y.h) return x.h > y.h;
    if (x.h == 0) return false;
    return x.i < y.i || (x.i == y.i && x.j < y.j);
}

// The walk back from the best cell (thread 0), both gap models: H's source
// in bits 0-1 of a direction byte, E / F extending in bits 2 / 3 (always 0
// under linear gaps, where every E / F opens).  The walk meets the path's
// last op first, so it runs twice when ops are wanted: once to count the
// path and find the begin cell, then again storing step n (from the end) at
// ops[len - 1 - n] where that lies inside the slot: a slot shorter than the
// path holds the path's first ops_stride ops, from the begin cell.
//
// The hit's query-anchored row (AlignArgs::msa, filled with kMsaNone by
// align_row_clear before the sweep) is written in the first pass, where the
// path is known cell by cell: an M at (i, j) puts subject residue s[j-1] at
// position i-1, an I puts kMsaGap there, a D has no query position.  The row
// has one byte per query position, so no slot can truncate it.
__device__ void align_walk(const AlignArgs& a, const Best& bb, const uint8_t* T, int W1, int hit,
                           const uint8_t* __restrict__ s) {
    char* ops = a.ops ? a.ops + static_cast<int64_t>(hit) * a.ops_stride : nullptr;
    uint8_t* row = a.msa ? a.msa + static_cast<int64_t>(hit) * a.qlen : nullptr;
    int i = 0, j = 0;
    int64_t len = 0;
    for (int pass = 0; pass < (ops ? 2 : 1); ++pass) {
        int state = 0;  // 0: H, 1: in an E run (left), 2: in an F run (up)
        int64_t n = 0;
        i = bb.i;
        j = bb.j;
        while (i > 0 && j > 0) {
            const int t = T[static_cast<int64_t>(i + j) * W1 + i];
            char op;
            if (state == 0) {
                const int src = t & 3;
                if (src == 0) break;  // a zero cell (H = 0 has no source)
                if (src != 3) {
                    state = src;
                    continue;
                }
                op = 'M';
                if (row && !pass) row[i - 1] = s[j - 1];
                --i;
                --j;
            } else if (state == 1) {
                op = 'D';
                state = (t & 4) ? 1 : 0;
                --j;
            } else {
                op = 'I';
                state = (t & 8) ? 2 : 0;
                if (row && !pass) row[i - 1] = kMsaGap;
                --i;
            }
            if (pass && len - 1 - n < a.ops_stride) ops[len - 1 - n] = op;
            ++n;
        }
        len = n;
    }
    const int64_t n = len;
    int32_t* r = a.out + static_cast<int64_t>(hit) * 6;
    r[0] = bb.h;
    r[1] = i + 1;  // q_begin (1-based)
    r[2] = bb.i;   // q_end
    r[3] = j + 1;  // s_begin
    r[4] = bb.j;   // s_end
    r[5] = static_cast<int32_t>(n);
}

// The hit's row of AlignArgs::msa starts as all kMsaNone (every thread, before
// the sweep's first barrier; the walk's writes follow the last one).
__device__ __forceinline__ void align_row_clear(const AlignArgs& a, int hit, int tid) {
    if (!a.msa) return;
    uint8_t* row = a.msa + static_cast<int64_t>(hit) * a.qlen;
    for (int k = tid; k < a.qlen; k += kAlignThreads) row[k] = kMsaNone;
}

// The diagonal term's score S(query row i, subject code c), i 1-based: the two
// forms of a query.  MatScore: a residue sequence against the 25 x 25 matrix
// staged in LDS.  PssmScore: a position-specific table, read from the resident
// transposed image (PssmProfileArgs) in global memory; no LDS table is staged.
struct MatScore {
    static constexpr bool kStaged = true;
    const int8_t* smat;
    const uint8_t* __restrict__ q;
    __device__ MatScore(const AlignArgs& a, const int8_t* lds) : smat(lds), q(a.query) {}
    __device__ __forceinline__ int operator()(int i, int c) const { return smat[25 * q[i - 1] + c]; }
};
struct PssmScore {
    static constexpr bool kStaged = false;
    const int8_t* __restrict__ t;
    int ld;
    __device__ PssmScore(const AlignArgs& a, const int8_t*) : t(a.pssm), ld(a.pssm_ld) {}
    __device__ __forceinline__ int operator()(int i, int c) const { return t[static_cast<int64_t>(c) * ld + i - 1]; }
};

template <class Score>
__global__ __launch_bounds__(kAlignThreads) void sw_align_linear(AlignArgs a) {
    __shared__ int8_t smat[Score::kStaged ? 640 : 16];
    __shared__ Best red[kAlignThreads];
    const int hit = blockIdx.x;
    const int tid = threadIdx.x;
    const int qlen = a.qlen;
    const int64_t soff = a.subj_off[hit];
    const int slen = static_cast<int>(a.subj_off[hit + 1] - soff);
    const uint8_t* __restrict__ s = a.subj + soff;
    const int W1 = qlen + 1;
    int32_t* Hb = a.hbuf + static_cast<int64_t>(hit) * 3 * W1;
    uint8_t* T = a.dirs + a.dirs_off[hit];
    const int gap = a.gap;
    const Score score(a, smat);

    if constexpr (Score::kStaged)
        for (int k = tid; k < 625; k += kAlignThreads) smat[k] = a.mat[k];
    for (int k = tid; k < 3 * W1; k += kAlignThreads) Hb[k] = 0;
    align_row_clear(a, hit, tid);
    __syncthreads();

    Best b = {0, 0, 0};
    for (int d = 2; d <= qlen + slen; ++d) {
        const int lo = max(1, d - slen);
        const int hi = min(qlen, d - 1);
        int32_t* cur = Hb + (d % 3) * W1;
        const int32_t* p1 = Hb + ((d + 2) % 3) * W1;  // diagonal d-1
        const int32_t* p2 = Hb + ((d + 1) % 3) * W1;  // diagonal d-2
        for (int i = lo + tid; i <= hi; i += kAlignThreads) {
            const int j = d - i;
            int h = 0, t = 0;
            const int left = p1[i] - gap;  // H(i, j-1)
            if (left > h) { h = left; t = 1; }
            const int up = p1[i - 1] - gap;  // H(i-1, j)
            if (up > h) { h = up; t = 2; }
            const int dg = p2[i - 1] + score(i, s[j - 1]);  // H(i-1, j-1) + S
            if (dg > h) { h = dg; t = 3; }
            cur[i] = h;
            T[static_cast<int64_t>(d) * W1 + i] = static_cast<uint8_t>(t);
            const Best c = {h, i, j};
            if (better(c, b)) b = c;
        }
        __syncthreads();  // diagonal d complete before d+1 reads it
    }

    red[tid] = b;
    __syncthreads();
    for (int w = kAlignThreads / 2; w > 0; w >>= 1) {
        if (tid < w && better(red[tid + w], red[tid])) red[tid] = red[tid + w];
        __syncthreads();
    }
    if (tid == 0) align_walk(a, red[0], T, W1, hit, s);
}

// Affine gaps (Gotoh; a k-gap costs gap + (k - 1) gap_extend).  The reference
// has no affine traceback, so the tie order is this build's own, cpu.cpp's
// carried over (oracle swo_align_affine states the same): E(i,j) opens from
// H(i,j-1) unless extending E(i,j-1) is STRICTLY better (F likewise down the
// column), H takes E, then F, then the diagonal on strict improvements over
// 0, the first strict maximum in row-major order ends the alignment.  The
// sweep keeps three diagonals of H and two of E and F (7 x (qlen + 1) int32
// per hit); E(i,j) reads diagonal d-1 at i, F(i,j) at i-1.
template <class Score>
__global__ __launch_bounds__(kAlignThreads) void sw_align_affine(AlignArgs a) {
    __shared__ int8_t smat[Score::kStaged ? 640 : 16];
    __shared__ Best red[kAlignThreads];
    constexpr int NEG = -(1 << 29);
    const int hit = blockIdx.x;
    const int tid = threadIdx.x;
    const int qlen = a.qlen;
    const int64_t soff = a.subj_off[hit];
    const int slen = static_cast<int>(a.subj_off[hit + 1] - soff);
    const uint8_t* __restrict__ s = a.subj + soff;
    const Score score(a, smat);
    const int W1 = qlen + 1;
    int32_t* Hb = a.hbuf + static_cast<int64_t>(hit) * 7 * W1;
    int32_t* Eb = Hb + 3 * W1;
    int32_t* Fb = Eb + 2 * W1;
    uint8_t* T = a.dirs + a.dirs_off[hit];
    const int go = a.gap, ge = a.gap_extend;

    if constexpr (Score::kStaged)
        for (int k = tid; k < 625; k += kAlignThreads) smat[k] = a.mat[k];
    for (int k = tid; k < 3 * W1; k += kAlignThreads) Hb[k] = 0;
    align_row_clear(a, hit, tid);
    for (int k = tid; k < 4 * W1; k += kAlignThreads) Eb[k] = NEG;  // E and F
    __syncthreads();

    Best b = {0, 0, 0};
    for (int d = 2; d <= qlen + slen; ++d) {
        const int lo = max(1, d - slen);
        const int hi = min(qlen, d - 1);
        int32_t* cur = Hb + (d % 3) * W1;
        const int32_t* p1 = Hb + ((d + 2) % 3) * W1;  // H, diagonal d-1
        const int32_t* p2 = Hb + ((d + 1) % 3) * W1;  // H, diagonal d-2
        int32_t* ec = Eb + (d & 1) * W1;
        const int32_t* ep = Eb + ((d + 1) & 1) * W1;  // E, diagonal d-1
        int32_t* fc = Fb + (d & 1) * W1;
        const int32_t* fp = Fb + ((d + 1) & 1) * W1;  // F, diagonal d-1
        for (int i = lo + tid; i <= hi; i += kAlignThreads) {
            const int j = d - i;
            int t = 0;
            int e = p1[i] - go;                           // open from H(i, j-1)
            if (ep[i] - ge > e) { e = ep[i] - ge; t |= 4; }  // extend E(i, j-1)
            int f = p1[i - 1] - go;                       // open from H(i-1, j)
            if (fp[i - 1] - ge > f) { f = fp[i - 1] - ge; t |= 8; }
            int h = 0;
            if (e > h) { h = e; t = (t & 12) | 1; }
            if (f > h) { h = f; t = (t & 12) | 2; }
            const int dg = p2[i - 1] + score(i, s[j - 1]);
            if (dg > h) { h = dg; t = (t & 12) | 3; }
            cur[i] = h;
            ec[i] = e;
            fc[i] = f;
            T[static_cast<int64_t>(d) * W1 + i] = static_cast<uint8_t>(t);
            const Best c = {h, i, j};
            if (better(c, b)) b = c;
        }
        __syncthreads();  // diagonal d complete before d+1 reads it
    }

    red[tid] = b;
    __syncthreads();
    for (int w = kAlignThreads / 2; w > 0; w >>= 1) {
        if (tid < w && better(red[tid + w], red[tid])) red[tid] = red[tid + w];
        __syncthreads();
    }
    if (tid == 0) align_walk(a, red[0], T, W1, hit, s);
}

hipError_t launch_align(const AlignArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const bool affine = a.gap_extend != a.gap;
    if (a.pssm) {
        if (a.pssm_ld < a.qlen) return hipErrorInvalidValue;
        if (affine)
            hipLaunchKernelGGL(sw_align_affine<PssmScore>, dim3(a.n), dim3(kAlignThreads), 0, s, a);
        else
            hipLaunchKernelGGL(sw_align_linear<PssmScore>, dim3(a.n), dim3(kAlignThreads), 0, s, a);
    } else if (affine) {
        hipLaunchKernelGGL(sw_align_affine<MatScore>, dim3(a.n), dim3(kAlignThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(sw_align_linear<MatScore>, dim3(a.n), dim3(kAlignThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace swk
