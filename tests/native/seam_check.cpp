// seam_check.cpp — a stand-alone restatement of the local-alignment score
// (Gotoh's affine recurrence; open == extend is the linear one) that can
// mis-carry ONE quantity across ONE seam of the DP matrix, for
// tests/test_seam_probes.py: what would a scan kernel's error at a strip,
// pass, lane or column-group seam do to the scores of the seam probes?
//
//   E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)      along a row
//   F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)      down a column
//   H[i][j] = max(0, H[i-1][j-1] + S[q_i][s_j], E[i][j], F[i][j])
//
// A row seam r is the step from row r - 1 to row r (0-based), a column seam c
// the step from column c - 1 to column c.  At the seam one of the two terms
// of F (rows) or E (columns) is changed in every column (row):
//   fault 0, 1, 2: the gap state's carry  F[r-1][j] - ge  dropped, + ge, - ge
//   fault 3, 4, 5: the opening source     H[r-1][j] - go  dropped, + ge, - ge
//
// Input (a text file, argv[1]; every number separated by white space):
//   nm, then nm matrices of 625 entries (row = query code)
//   ns, then ns scorings: matrix index, open, extend
//   the query: n, then n codes
//   np, then np subjects: n, then n codes
//   nt, then nt tasks: scoring, axis (0 rows, 1 columns), seam, fault, count, then count subject indices
// Output: one line "base <scoring>" + the np fault-free scores per scoring;
// then per task "task <first subject of the list whose score the fault
// changes, or -1> <its faulty score> <subjects tried>".
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <thread>
#include <vector>

namespace {

constexpr int kNone = -(1 << 28);  // "no gap state": below everything, far from overflow

struct Scoring {
    int mat = 0, go = 0, ge = 0;
};

int faulty(int v, int fault, int ge) {
    switch (fault % 3) {
    case 0: return kNone;
    case 1: return v + ge;
    default: return v - ge;
    }
}

// AXIS < 0: no fault, 0: a row seam, 1: a column seam
template <int AXIS>
int score_at(const std::vector<int>& q, const std::vector<int>& s, const int* mat, int go, int ge, int seam, int fault) {
    const int n = static_cast<int>(s.size());
    std::vector<int> H(n + 1, 0), F(n + 1, kNone);
    int best = 0;
    for (int i = 0; i < static_cast<int>(q.size()); ++i) {
        const int* row = mat + 25 * q[i];
        const bool rs = AXIS == 0 && i == seam;
        int diag = 0, left = 0, e = kNone;  // H[i-1][j-1], H[i][j-1], E[i][j-1]
        for (int j = 0; j < n; ++j) {
            int fc = std::max(F[j + 1] - ge, kNone), fo = H[j + 1] - go;
            if (rs && fault < 3) fc = faulty(fc, fault, ge);
            if (rs && fault >= 3) fo = faulty(fo, fault, ge);
            int ec = std::max(e - ge, kNone), eo = left - go;
            if (AXIS == 1 && j == seam) {
                if (fault < 3) ec = faulty(ec, fault, ge);
                else eo = faulty(eo, fault, ge);
            }
            const int f = std::max(fc, fo);
            e = std::max(ec, eo);
            const int h = std::max(std::max(0, diag + row[s[j]]), std::max(e, f));
            diag = H[j + 1];
            H[j + 1] = h;
            F[j + 1] = f;
            left = h;
            best = std::max(best, h);
        }
    }
    return best;
}

int score(const std::vector<int>& q, const std::vector<int>& s, const int* mat, int go, int ge, int axis, int seam,
          int fault) {
    if (axis == 0) return score_at<0>(q, s, mat, go, ge, seam, fault);
    if (axis == 1) return score_at<1>(q, s, mat, go, ge, seam, fault);
    return score_at<-1>(q, s, mat, go, ge, 0, 0);
}

// f(k) for k in [0, n) on the machine's threads (at most 16)
template <class Fn>
void parallel(int n, Fn f) {
    const int nt = static_cast<int>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&] {
            for (int k = next++; k < n; k = next++) f(k);
        });
    for (auto& t : pool) t.join();
}

std::vector<int> read_seq(std::istream& in) {
    int n = 0;
    in >> n;
    std::vector<int> v(static_cast<size_t>(std::max(n, 0)));
    for (int& x : v) in >> x;
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: seam_check INPUT\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    int nm = 0, ns = 0, np = 0, nt = 0;
    in >> nm;
    std::vector<int> mats(static_cast<size_t>(nm) * 625);
    for (int& x : mats) in >> x;
    in >> ns;
    std::vector<Scoring> sc(static_cast<size_t>(ns));
    for (Scoring& s : sc) in >> s.mat >> s.go >> s.ge;
    const std::vector<int> q = read_seq(in);
    in >> np;
    std::vector<std::vector<int>> subs(static_cast<size_t>(np));
    for (auto& s : subs) s = read_seq(in);
    in >> nt;
    if (!in || nm < 1 || ns < 1) {
        std::fprintf(stderr, "seam_check: malformed input\n");
        return 2;
    }
    for (int x : q)
        if (x < 0 || x > 24) return 2;
    for (const auto& s : subs)
        for (int x : s)
            if (x < 0 || x > 24) return 2;
    std::vector<std::vector<int>> base(static_cast<size_t>(ns), std::vector<int>(static_cast<size_t>(np)));
    for (int k = 0; k < ns; ++k) {
        if (sc[k].mat < 0 || sc[k].mat >= nm) return 2;
        parallel(np, [&](int p) { base[k][p] = score(q, subs[p], &mats[625 * sc[k].mat], sc[k].go, sc[k].ge, -1, 0, 0); });
        std::printf("base %d", k);
        for (int p = 0; p < np; ++p) std::printf(" %d", base[k][p]);
        std::printf("\n");
    }
    struct Task {
        int k = 0, axis = 0, seam = 0, fault = 0;
        std::vector<int> subjects;
        int hit = -1, hit_score = 0, tried = 0;
    };
    std::vector<Task> tasks(static_cast<size_t>(std::max(nt, 0)));
    for (int t = 0; t < nt; ++t) {
        Task& T = tasks[t];
        int cnt = 0;
        in >> T.k >> T.axis >> T.seam >> T.fault >> cnt;
        if (!in || T.k < 0 || T.k >= ns || T.axis < 0 || T.axis > 1 || T.fault < 0 || T.fault > 5 || cnt < 0) {
            std::fprintf(stderr, "seam_check: malformed task %d\n", t);
            return 2;
        }
        T.subjects.resize(static_cast<size_t>(cnt));
        for (int& p : T.subjects) {
            in >> p;
            if (!in || p < 0 || p >= np) return 2;
        }
    }
    parallel(nt, [&](int t) {
        Task& T = tasks[t];
        const Scoring& s = sc[T.k];
        for (int p : T.subjects) {
            ++T.tried;
            const int v = score(q, subs[p], &mats[625 * s.mat], s.go, s.ge, T.axis, T.seam, T.fault);
            if (v != base[T.k][p]) {
                T.hit = p;
                T.hit_score = v;
                break;
            }
        }
    });
    for (const Task& T : tasks) std::printf("task %d %d %d\n", T.hit, T.hit_score, T.tried);
    std::printf("seam_check ok\n");
    return 0;
}
