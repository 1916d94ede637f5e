// sw_hits.hip — the hit table (sw_hit_stats / sw_scan_hits, sw_amd.h): for
// each chosen hit, where sw_align's alignment lies and its length,
// identities, positives and gaps, in ONE forward pass with no direction
// matrix and no walk back.
//
// One workgroup of W waves per hit, each wave in the shape of sw_intra
// (sw_int32.h intra_subject): thread t owns query rows [t RI, (t + 1) RI) of a
// 64 W RI-row chunk, lane l of a wave handles subject column k - l at the
// wave's step k; its bottom row moves down a lane by DPP wave_shr:1.  Lane 0
// of wave 0 is fed from the previous chunk's boundary row (device memory),
// lane 0 of a later wave from the wave above through an LDS ring, and the
// last wave's lane 63 writes the next chunk's boundary row.  (One wave of 8
// rows per lane was the first form: a hit's latency is its serial wavefront,
// and W = 4 waves of 2 rows cut the step to a third.)  Each of H and E (per row, in
// registers), F (moving down the column) and the diagonal is a swhits::Cell:
// an int32 value and the path that produced it (begin cell, length,
// identities, positives, gap runs, last op), chosen by sw_hits_rules.h's
// gap_step / cell_step, the same code the CPU check runs.  The best cell is
// the first strict maximum in row-major order: each thread keeps its own (its
// columns ascend, so on equal values only a smaller row wins), and the
// workgroup reduces (value, row, column).
//
// A hit is a (query, subject) pair (HitDesc): one launch may mix queries of
// any lengths (sw_hit_stats_batch), one-chunk hits, which never touch the
// scratch, beside multi-chunk ones, and empty queries; the host orders the
// grid (swplan::hits_order) and each hit writes the row its descriptor names.
//
// The subject is read where the scan kernels read it, in the resident packed
// database (HitDesc, hit_residue_at): no residue is uploaded.  Codes there
// are stored codes (kStored), so the per-chunk LDS profile is built in stored
// order (its columns through kCodeOf) and identity compares the query's
// stored code with the subject's.  Scratch is the chunk boundary row alone,
// kHitsBndWords int32 per subject column, and only for queries longer than a
// chunk.  Padding rows (>= qlen) and columns (>= slen) score 0, never feed a
// real cell (values move right and down only) and are kept out of the
// maximum.
#include "sw_hits_rules.h"
#include "sw_kernels.h"

namespace swk {

namespace {

using swhits::Cell;
using swhits::kNeg;
using swhits::kOpD;
using swhits::kOpI;
using swhits::Path;

// DPP wave_shr:1: lane t gets lane t - 1's src; lane 0 keeps `old`
__device__ __forceinline__ int hits_shr1(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ Cell hits_shr1(const Cell& old, const Cell& src) {
    Cell c;
    c.v = hits_shr1(old.v, src.v);
    c.p.i0 = hits_shr1(old.p.i0, src.p.i0);
    c.p.j0 = hits_shr1(old.p.j0, src.p.j0);
    c.p.len = hits_shr1(old.p.len, src.p.len);
    c.p.ident = hits_shr1(old.p.ident, src.p.ident);
    c.p.pos = hits_shr1(old.p.pos, src.p.pos);
    c.p.opens = hits_shr1(old.p.opens, src.p.opens);
    c.p.last = hits_shr1(old.p.last, src.p.last);
    return c;
}
__device__ __forceinline__ int hits_sx8(uint32_t w, int b) { return static_cast<int>(static_cast<int8_t>(w >> (8 * b))); }

}  // namespace

template <int RI, int W>
__global__ __launch_bounds__(kLanes * W) void sw_hits(HitArgs a) {
    constexpr int T = kLanes * W;           // threads: one per RI query rows of a chunk
    constexpr int CH = T * RI;              // query rows per chunk
    constexpr int RIP = (RI + 3) / 4 * 4;   // bytes of a thread's profile slot
    constexpr int S = T * RIP + 4;          // + 4: threads reading different codes start on different banks
    constexpr int NCODE = kPadCode + 1;
    constexpr int RING = 2 * kLanes;        // columns of a wave-to-wave ring
    static_assert(CH == kHitsChunkRows, "the host sizes the boundary rows by kHitsChunkRows");
    __shared__ __attribute__((aligned(16))) uint8_t prof[NCODE * S];  // [stored code][thread][RIP]
    __shared__ int8_t smat[kAlphabet * kAlphabet + 15];
    // wave w's bottom row for wave w + 1: column c at slot c % RING, kHitsBndWords int32 as in HitArgs::bnd
    __shared__ int4 ring[W > 1 ? W - 1 : 1][RING][kHitsBndWords / 4];
    __shared__ int red[W][3];

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & (kLanes - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kLanes);
    const int hit = static_cast<int>(blockIdx.x);
    const HitDesc d = a.hits[hit];
    // the query is the hit's own: everything below that depends on it (the
    // chunk loop, wact, first / last, the padding rows, the profile, whether
    // bnd is touched) follows d.qlen, uniform over the workgroup
    const int L = d.slen, qlen = d.qlen;
    const uint8_t* __restrict__ query = a.query + d.qoff;
    sw_hit* const o = a.out + d.row;
    if (tid == 0) {
        o->id = d.id;
        o->s_len = d.slen;
    }
    if (L <= 0 || qlen <= 0) {
        if (tid == 0) swhits::zero_row(*o);
        return;
    }
    const uint8_t* __restrict__ sp = d.lane < 0 ? a.lres + a.loff[d.slot] : a.res + a.blk_off[d.slot];
    int32_t* const bnd = a.bnd + d.scratch * kHitsBndWords;  // touched only when qlen > CH
    const int go = a.gap_open, ge = a.gap_extend;
    for (int k = tid; k < kAlphabet * kAlphabet; k += T) smat[k] = a.mat[k];

    int bv = 0, bi = 0, bj = 0;  // this thread's best cell and its path
    Path bp = swhits::cell_of(0).p;
    const int nsteps = L + kLanes - 1;                    // of a wave: lane l handles column step - l
    const int nblk = (nsteps + kLanes - 1) / kLanes;      // blocks of 64 steps

    for (int c0 = 0; c0 < qlen; c0 += CH) {
        const bool first = c0 == 0;
        const bool last = c0 + CH >= qlen;
        // waves that hold a query row in this chunk (all of them but in the last chunk)
        const int wact = min(W, (min(qlen - c0, CH) + kLanes * RI - 1) / (kLanes * RI));
        const int row1 = c0 + tid * RI + 1;  // 1-based query row of this thread's row 0
        __syncthreads();  // the matrix is staged; the previous chunk's profile and ring reads are done
        int qst[RI];      // the rows' stored codes (255: a padding row)
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            const int row = row1 - 1 + r;
            const int qc = row < qlen ? query[row] : 255;
            qst[r] = qc < kAlphabet ? kStored[qc] : 255;
            for (int c = 0; c < NCODE; ++c)
                prof[c * S + tid * RIP + r] =
                    static_cast<uint8_t>((qc < kAlphabet && c < kAlphabet) ? smat[kAlphabet * qc + kCodeOf[c]] : 0);
        }
        __syncthreads();

        Cell H[RI], E[RI];
#pragma unroll
        for (int r = 0; r < RI; ++r) {
            H[r] = swhits::cell_of(0);
            E[r] = swhits::cell_of(kNeg, kOpD);
        }
        Cell hl = swhits::cell_of(0), fl = swhits::cell_of(kNeg, kOpI);  // the bottom row's H, F at this lane's last column
        Cell up_prev = swhits::cell_of(0);  // H of the row above at column j - 1 (row 0's diagonal)
        int rc = kPadCode;                  // stored code of this lane's current column
        const uint8_t* const lrow = prof + tid * RIP;
        // wave 0's top row is the previous chunk's bottom row (device memory), a
        // later wave's the bottom row of the wave above (its ring)
        const bool has_top = wave > 0 || !first;

        // Wave w runs its block b (steps 64 b .. 64 b + 63) in round b + 2 w:
        // its top row for columns 64 b .. 64 b + 63 left lane 63 of wave w - 1
        // at that wave's steps 64 b + 63 .. 64 b + 126, blocks b and b + 1,
        // rounds b + 2 w - 2 and b + 2 w - 1.  Two barriers per round: the
        // rings are read (into registers) before the round's writes, so a slot
        // written at the end of a round is not one still to be read in it.
        for (int t = 0; t < nblk + 2 * (wact - 1); ++t) {
            const int b = t - 2 * wave;
            const bool active = wave < wact && b >= 0 && b < nblk;
            const int k0 = b * kLanes;
            // lane 0's inputs for steps k0 .. k0 + 63 (column = step), one column per lane
            const int ccol = k0 + lane;
            int in_res = kPadCode;
            int inb[kHitsBndWords];
#pragma unroll
            for (int w = 0; w < kHitsBndWords; ++w) inb[w] = (w == 8) ? kNeg : 0;
            if (active && ccol < L) {
                in_res = sp[hit_residue_at(d.lane, static_cast<uint64_t>(ccol))];
                if (has_top) {
                    const int4* src = wave > 0 ? &ring[wave - 1][ccol & (RING - 1)][0]
                                               : reinterpret_cast<const int4*>(bnd + static_cast<int64_t>(ccol) * kHitsBndWords);
#pragma unroll
                    for (int w = 0; w < kHitsBndWords / 4; ++w) {
                        const int4 v = src[w];
                        inb[4 * w] = v.x; inb[4 * w + 1] = v.y; inb[4 * w + 2] = v.z; inb[4 * w + 3] = v.w;
                    }
                }
            }
            if (W > 1) __syncthreads();
            const int mend = active ? min(kLanes, nsteps - k0) : 0;
            for (int m = 0; m < mend; ++m) {
                const int k = k0 + m;
                rc = hits_shr1(__builtin_amdgcn_readlane(in_res, m), rc);
                Cell top_h = swhits::cell_of(0), top_f = swhits::cell_of(kNeg, kOpI);
                if (has_top) {
                    top_h.v = __builtin_amdgcn_readlane(inb[0], m);
                    top_h.p.i0 = __builtin_amdgcn_readlane(inb[1], m);
                    top_h.p.j0 = __builtin_amdgcn_readlane(inb[2], m);
                    top_h.p.len = __builtin_amdgcn_readlane(inb[3], m);
                    top_h.p.ident = __builtin_amdgcn_readlane(inb[4], m);
                    top_h.p.pos = __builtin_amdgcn_readlane(inb[5], m);
                    top_h.p.opens = __builtin_amdgcn_readlane(inb[6], m);
                    top_h.p.last = __builtin_amdgcn_readlane(inb[7], m);
                    top_f.v = __builtin_amdgcn_readlane(inb[8], m);
                    top_f.p.i0 = __builtin_amdgcn_readlane(inb[9], m);
                    top_f.p.j0 = __builtin_amdgcn_readlane(inb[10], m);
                    top_f.p.len = __builtin_amdgcn_readlane(inb[11], m);
                    top_f.p.ident = __builtin_amdgcn_readlane(inb[12], m);
                    top_f.p.pos = __builtin_amdgcn_readlane(inb[13], m);
                    top_f.p.opens = __builtin_amdgcn_readlane(inb[14], m);
                }
                const Cell up0 = hits_shr1(top_h, hl);
                Cell f = hits_shr1(top_f, fl);
                f.p.last = kOpI;  // an F path ends in I (the rows above, or the initial value)
                const uint32_t* pp = reinterpret_cast<const uint32_t*>(lrow + rc * S);
                uint32_t pw[RIP / 4];
#pragma unroll
                for (int q = 0; q < RIP / 4; ++q) pw[q] = pp[q];
                const int col = k - lane;
                const bool colok = static_cast<unsigned>(col) < static_cast<unsigned>(L);
                Cell up = up0, diag = up_prev;
                up_prev = up0;
#pragma unroll
                for (int r = 0; r < RI; ++r) {
                    const int sc = hits_sx8(pw[r >> 2], r & 3);
                    const int i = row1 + r;
                    const Cell e = swhits::gap_step(E[r], H[r], go, ge, kOpD);
                    f = swhits::gap_step(f, up, go, ge, kOpI);
                    const Cell h = swhits::cell_step(e, f, diag, sc, qst[r] == rc, i, col + 1);
                    diag = H[r];
                    H[r] = h;
                    E[r] = e;
                    up = h;
                    // first strict maximum in row-major order: this thread's columns
                    // ascend, so an equal value wins only from a smaller row
                    if (colok && i <= qlen && (h.v > bv || (h.v == bv && i < bi))) {
                        bv = h.v;
                        bi = i;
                        bj = col + 1;
                        bp = h.p;
                    }
                }
                hl = up;
                fl = f;
                if (lane == kLanes - 1 && colok && (wave < wact - 1 || !last)) {
                    // lane 63 finished column k - 63 of its wave's bottom row: the top row
                    // of the wave below, or (the chunk's bottom row) of the next chunk
                    int4* dst = wave < wact - 1 ? &ring[wave][col & (RING - 1)][0]
                                                : reinterpret_cast<int4*>(bnd + static_cast<int64_t>(col) * kHitsBndWords);
                    dst[0] = make_int4(hl.v, hl.p.i0, hl.p.j0, hl.p.len);
                    dst[1] = make_int4(hl.p.ident, hl.p.pos, hl.p.opens, hl.p.last);
                    dst[2] = make_int4(fl.v, fl.p.i0, fl.p.j0, fl.p.len);
                    dst[3] = make_int4(fl.p.ident, fl.p.pos, fl.p.opens, 0);
                }
            }
            if (W > 1) __syncthreads();
        }
    }

    // the best cell: larger value, then smaller row, then smaller column
    auto better = [](int ov, int oi, int oj, int wv, int wi, int wj) {
        return ov > wv || (ov == wv && ov > 0 && (oi < wi || (oi == wi && oj < wj)));
    };
    int wv = bv, wi = bi, wj = bj;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int ov = __shfl_xor(wv, off), oi = __shfl_xor(wi, off), oj = __shfl_xor(wj, off);
        if (better(ov, oi, oj, wv, wi, wj)) {
            wv = ov;
            wi = oi;
            wj = oj;
        }
    }
    if (lane == 0) {
        red[wave][0] = wv;
        red[wave][1] = wi;
        red[wave][2] = wj;
    }
    __syncthreads();
    wv = red[0][0]; wi = red[0][1]; wj = red[0][2];
#pragma unroll
    for (int w = 1; w < W; ++w)
        if (better(red[w][0], red[w][1], red[w][2], wv, wi, wj)) {
            wv = red[w][0];
            wi = red[w][1];
            wj = red[w][2];
        }
    if (wv <= 0) {
        if (tid == 0) swhits::zero_row(*o);
    } else if (bv == wv && bi == wi && bj == wj) {
        swhits::fill_row(*o, bv, bi, bj, bp);
    }
}

hipError_t launch_hits(const HitArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.qlen_max > kHitsChunkRows && !a.bnd) return hipErrorInvalidValue;
    hipLaunchKernelGGL((sw_hits<kHitsRowsPerLane, kHitsWaves>), dim3(a.n), dim3(kLanes * kHitsWaves), 0, s, a);
    return hipGetLastError();
}

}  // namespace swk
