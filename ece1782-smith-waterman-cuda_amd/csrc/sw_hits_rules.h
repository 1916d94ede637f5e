// sw_hits_rules.h — the hit table's carried-tuple rules (sw_hit, sw_amd.h),
// shared by the kernel (sw_hits.hip) and by the scalar pass below, which
// tests/native/hits_check.cpp pins to the oracle's traceback.  No HIP call.
//
// Every column of a sw_hit row is additive along the alignment path, so no
// direction matrix is kept: each of H, E and F carries, beside its value, the
// begin cell and the counters of the path that produced it, and takes them
// from whichever source sw_align's tie rules pick (sw_align.hip, oracle
// swo_align_affine).  The best cell's tuple is then what the walk back would
// have found.  One set of rules serves both gap models: with gap_open ==
// gap_extend an extension is never strictly better than opening from H, so
// E / F always take H's tuple, which is sw_align_linear's left / up.
#pragma once

#include <stdint.h>

#include "sw_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SWH_FN __host__ __device__ __forceinline__
#else
#define SWH_FN inline
#endif

namespace swhits {

// the last column of a path: none (no path), an aligned pair, a subject
// residue against a gap (E, along the row), a query residue against a gap (F)
enum : int32_t { kOpNone = 0, kOpM = 1, kOpD = 2, kOpI = 3 };

// E and F of the cells before the first row / column, as sw_align_affine's
constexpr int32_t kNeg = -(1 << 29);

struct Path {
    int32_t i0, j0;  // begin cell, 1-based
    int32_t len;     // alignment columns
    int32_t ident;   // M columns whose two residue codes are equal
    int32_t pos;     // M columns whose matrix entry is > 0
    int32_t opens;   // maximal runs of I or of D
    int32_t last;    // kOp* of the path's last column
};
struct Cell {
    int32_t v;
    Path p;
};

SWH_FN Cell cell_of(int32_t v, int32_t last = kOpNone) { return Cell{v, Path{0, 0, 0, 0, 0, 0, last}}; }

// The faults tests/native/hits_check.cpp injects (each must change some row):
// 1 the last op is not carried when a run opens from H, 2 H takes F's begin
// cell when F ties with E, 3 positives count entries >= 0.
enum : int { kFaultNone = 0, kFaultLastOp = 1, kFaultTieBegin = 2, kFaultPositives = 3 };

// E(i,j) from E(i,j-1) (run) and H(i,j-1) (h) with op = kOpD; F(i,j) from
// F(i-1,j) and H(i-1,j) with op = kOpI: the run's tuple if extending is
// STRICTLY better, else H's; then one gap column, which opens a run unless
// the source's path already ends in this op.
template <int FAULT = kFaultNone>
SWH_FN Cell gap_step(const Cell& run, const Cell& h, int32_t go, int32_t ge, int32_t op) {
    const int32_t ext = run.v - ge, opn = h.v - go;
    const bool extend = ext > opn;
    Cell c;
    c.v = extend ? ext : opn;
    c.p = extend ? run.p : h.p;
    if (FAULT == kFaultLastOp && !extend) c.p.last = kOpNone;
    c.p.opens += c.p.last != op ? 1 : 0;
    c.p.len += 1;
    c.p.last = op;
    return c;
}

// H(i,j): 0 with no path, then E, then F, then the diagonal, each only on a
// strict improvement.  s = the matrix entry of (query row i, subject column
// j), same = their residue codes are equal.  A diagonal step from a zero
// cell starts a path at (i, j).
template <int FAULT = kFaultNone>
SWH_FN Cell cell_step(const Cell& e, const Cell& f, const Cell& diag, int32_t s, bool same, int32_t i, int32_t j) {
    Cell h = cell_of(0);
    if (e.v > h.v) h = e;
    if (f.v > h.v) {
        h = f;
    } else if (FAULT == kFaultTieBegin && f.v == h.v && f.v > 0) {
        h.p.i0 = f.p.i0;
        h.p.j0 = f.p.j0;
    }
    const int32_t dg = diag.v + s;
    if (dg > h.v) {
        h.v = dg;
        h.p = diag.p;
        if (diag.v == 0) h.p = Path{i, j, 0, 0, 0, 0, kOpNone};
        h.p.len += 1;
        h.p.ident += same ? 1 : 0;
        h.p.pos += (FAULT == kFaultPositives ? s >= 0 : s > 0) ? 1 : 0;
        h.p.last = kOpM;
    }
    return h;
}

// The row of the best cell (value v > 0 at (i, j), path p); id and s_len are
// the caller's.  gaps and the M count follow from the spans and the length:
// q span = M + I, s span = M + D, length = M + I + D.
SWH_FN void fill_row(sw_hit& o, int32_t v, int32_t i, int32_t j, const Path& p) {
    o.score = v;
    o.q_begin = p.i0;
    o.q_end = i;
    o.s_begin = p.j0;
    o.s_end = j;
    o.length = p.len;
    o.identities = p.ident;
    o.positives = p.pos;
    o.gap_opens = p.opens;
    o.gaps = 2 * p.len - (i - p.i0 + 1) - (j - p.j0 + 1);
}
// A hit of score 0 (an empty subject, an empty query): every field but id
// and s_len is 0.
SWH_FN void zero_row(sw_hit& o) {
    o.score = o.q_begin = o.q_end = o.s_begin = o.s_end = 0;
    o.length = o.identities = o.positives = o.gap_opens = o.gaps = 0;
}

}  // namespace swhits

#include <vector>

namespace swhits {

// The scalar pass: row-major over the matrix, O(slen) cells kept; the best
// cell is the first strict maximum in that order.  q, s: residue codes;
// mat: 25 x 25 (row = query code).  id and s_len of the row are left alone.
template <int FAULT = kFaultNone>
void scalar_pass(const uint8_t* q, int32_t qlen, const uint8_t* s, int32_t slen, const int8_t* mat, int32_t go,
                 int32_t ge, sw_hit& out) {
    zero_row(out);
    if (qlen <= 0 || slen <= 0) return;
    std::vector<Cell> H(static_cast<size_t>(slen) + 1, cell_of(0));   // row i - 1, then row i
    std::vector<Cell> F(static_cast<size_t>(slen) + 1, cell_of(kNeg, kOpI));
    int32_t bv = 0, bi = 0, bj = 0;
    Path bp = cell_of(0).p;
    for (int32_t i = 1; i <= qlen; ++i) {
        Cell diag = cell_of(0), left = cell_of(0), e = cell_of(kNeg, kOpD);
        for (int32_t j = 1; j <= slen; ++j) {
            e = gap_step<FAULT>(e, left, go, ge, kOpD);
            F[j] = gap_step<FAULT>(F[j], H[j], go, ge, kOpI);
            const int32_t sc = mat[25 * q[i - 1] + s[j - 1]];
            const Cell h = cell_step<FAULT>(e, F[j], diag, sc, q[i - 1] == s[j - 1], i, j);
            diag = H[j];
            H[j] = left = h;
            if (h.v > bv) {
                bv = h.v;
                bi = i;
                bj = j;
                bp = h.p;
            }
        }
    }
    if (bv > 0) fill_row(out, bv, bi, bj, bp);
}

}  // namespace swhits
