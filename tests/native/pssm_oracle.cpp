// pssm_oracle.cpp — a plain scalar restatement of Smith-Waterman under a
// position-specific scoring matrix, for the tests only (tests/test_pssm_oracle.py
// pins it to oracle/sw_oracle.c on derived tables before any GPU test relies
// on it; tests/test_gpu_pssm.py compares the library against it).
//
// rows is [qlen][25] int8: rows[25 i + c] = score of subject code c at query
// position i.  A gap of k residues costs go + (k - 1) ge; go == ge is the
// linear recurrence.  Traceback tie rules as oracle/sw_oracle.c states them:
// a cell takes left, then up, then the diagonal, each only on a strict
// improvement over the running value that starts at 0; a gap run opens
// unless extending it is strictly better; the end cell is the first strict
// maximum in row-major order; the walk back stops at a zero cell.
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace {

constexpr int kNeg = -(1 << 29);

int score_linear(const int8_t* rows, int qlen, const uint8_t* s, int slen, int gap) {
    std::vector<int> prev(static_cast<size_t>(slen) + 1, 0), cur(static_cast<size_t>(slen) + 1, 0);
    int best = 0;
    for (int i = 1; i <= qlen; ++i) {
        const int8_t* r = rows + 25 * static_cast<int64_t>(i - 1);
        cur[0] = 0;
        for (int j = 1; j <= slen; ++j) {
            int h = prev[j - 1] + r[s[j - 1]];
            if (cur[j - 1] - gap > h) h = cur[j - 1] - gap;
            if (prev[j] - gap > h) h = prev[j] - gap;
            if (h < 0) h = 0;
            cur[j] = h;
            if (h > best) best = h;
        }
        prev.swap(cur);
    }
    return best;
}

int score_affine(const int8_t* rows, int qlen, const uint8_t* s, int slen, int go, int ge) {
    // H and F of the previous row per column; E runs along the row
    std::vector<int> H(static_cast<size_t>(slen) + 1, 0), F(static_cast<size_t>(slen) + 1, kNeg);
    int best = 0;
    for (int i = 1; i <= qlen; ++i) {
        const int8_t* r = rows + 25 * static_cast<int64_t>(i - 1);
        int diag = 0, left = 0, e = kNeg;
        for (int j = 1; j <= slen; ++j) {
            const int up = H[j];
            e = (left - go > e - ge) ? left - go : e - ge;
            const int f = (up - go > F[j] - ge) ? up - go : F[j] - ge;
            int h = diag + r[s[j - 1]];
            if (e > h) h = e;
            if (f > h) h = f;
            if (h < 0) h = 0;
            F[j] = f;
            H[j] = h;
            diag = up;
            left = h;
            if (h > best) best = h;
        }
    }
    return best;
}

}  // namespace

extern "C" {

// out[k] = best local score of the table against subject k = res[offs[k] .. offs[k+1])
void pso_scan(const int8_t* rows, int qlen, const uint8_t* res, const int64_t* offs, int64_t n, int go, int ge,
              int32_t* out) {
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t* s = res + offs[k];
        const int slen = static_cast<int>(offs[k + 1] - offs[k]);
        out[k] = go == ge ? score_linear(rows, qlen, s, slen, go) : score_affine(rows, qlen, s, slen, go, ge);
    }
}

// Score and traceback.  pos = {q_end, s_end, q_begin, s_begin, ops_len}
// (1-based, inclusive; all 0 for an empty input); ops spells the path from the
// begin cell: 'M' pair, 'I' query position against a gap, 'D' subject residue
// against a gap.  go == ge is the linear traceback (every gap cell an opening).
int pso_align(const int8_t* rows, int qlen, const uint8_t* s, int slen, int go, int ge, int* pos, char* ops,
              int ops_cap) {
    for (int k = 0; k < 5; ++k) pos[k] = 0;
    if (qlen <= 0 || slen <= 0) return 0;
    const size_t W = static_cast<size_t>(slen) + 1, cells = (static_cast<size_t>(qlen) + 1) * W;
    std::vector<int> H(cells, 0), E(cells, kNeg), F(cells, kNeg);
    std::vector<unsigned char> T(cells, 0);  // bits 0-1: H's source (1 E, 2 F, 3 diagonal); 4: E extends; 8: F extends
    int best = 0, bi = 0, bj = 0;
    for (int i = 1; i <= qlen; ++i) {
        const int8_t* r = rows + 25 * static_cast<int64_t>(i - 1);
        for (int j = 1; j <= slen; ++j) {
            const size_t at = i * W + j;
            unsigned char t = 0;
            int e = H[at - 1] - go;
            if (E[at - 1] - ge > e) { e = E[at - 1] - ge; t |= 4; }
            int f = H[at - W] - go;
            if (F[at - W] - ge > f) { f = F[at - W] - ge; t |= 8; }
            int h = 0;
            if (e > h) { h = e; t = static_cast<unsigned char>((t & 12) | 1); }
            if (f > h) { h = f; t = static_cast<unsigned char>((t & 12) | 2); }
            const int d = H[at - W - 1] + r[s[j - 1]];
            if (d > h) { h = d; t = static_cast<unsigned char>((t & 12) | 3); }
            if (h > best) { best = h; bi = i; bj = j; }
            H[at] = h;
            E[at] = e;
            F[at] = f;
            T[at] = t;
        }
    }
    int i = bi, j = bj, n = 0, state = 0;  // 0: in H, 1: in an E run, 2: in an F run
    while (i > 0 && j > 0) {
        const unsigned char t = T[i * W + j];
        char op;
        if (state == 0) {
            const int src = t & 3;
            if (src == 0 || H[i * W + j] == 0) break;
            if (src != 3) { state = src; continue; }
            op = 'M'; --i; --j;
        } else if (state == 1) {
            op = 'D'; state = (t & 4) ? 1 : 0; --j;
        } else {
            op = 'I'; state = (t & 8) ? 2 : 0; --i;
        }
        if (n < ops_cap) ops[n] = op;
        ++n;
    }
    const int m = n < ops_cap ? n : ops_cap;
    for (int k = 0; k < m / 2; ++k) { const char c = ops[k]; ops[k] = ops[m - 1 - k]; ops[m - 1 - k] = c; }
    pos[0] = bi; pos[1] = bj; pos[2] = i + 1; pos[3] = j + 1; pos[4] = n;
    return best;
}

}  // extern "C"
