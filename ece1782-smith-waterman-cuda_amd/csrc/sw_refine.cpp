// sw_refine.cpp — the iterated profile search (include/sw_amd.h): the hits'
// query-anchored rows (sw_align.hip's walk back, through align_impl), their
// integer tables (sw_msa.hip), the step from tables to a PSSM
// (sw_pssm_build.cpp, host) and the loop around sw_search.cpp's scan, fit, key
// pass and selection.
#include <algorithm>
#include <cmath>
#include <iterator>

#include "sw_calib.h"
#include "sw_driver.h"
#include "sw_pssm_build.h"

using namespace swd;

namespace {

constexpr int32_t kMaxHits = SW_PROFILE_MAX_HITS;

// The matrix of the host-only calls: NULL is the reference's BLOSUM50.
int matrix_of(const int8_t* matrix, const int8_t** out) {
    const sw_scoring sc{matrix, 1, 1};
    int go, ge;
    return check_scoring(&sc, out, &go, &ge);
}

bool pseudo_ok(double pseudo) { return pseudo > 0 && pseudo <= 1000; }  // (false for NaN)

// The [qlen][25] table of a PSSM, from the image it keeps ([25][ld]).
void pssm_table(const sw_pssm* p, int8_t* rows) {
    for (int32_t i = 0; i < p->qlen; ++i)
        for (int c = 0; c < SW_ALPHABET; ++c)
            rows[static_cast<int64_t>(i) * SW_ALPHABET + c] = p->image[static_cast<size_t>(c) * p->ld + i];
}

// Step 1: rows[(n+1)][qlen] in device memory — the master (or all NONE), then
// the alignment of every ids[k] against p, written by the traceback's walk.
// The call returns after the last launch group has completed.
int build_rows(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t go, int32_t ge, const uint8_t* master,
               const int32_t* ids, int32_t n, DevPtr<uint8_t>& rows, sw_alignment* al) {
    if (int rc = check_pssm(h, p, go, ge)) return rc;
    if (!db || n < 0 || n > kMaxHits || (n > 0 && !ids)) return fail(SW_E_INVALID, "bad argument (0 <= n <= 4096)");
    if (db->h != h) return fail(SW_E_INVALID, "the database belongs to another handle");
    const int32_t qlen = p->qlen;
    for (int32_t i = 0; master && i < qlen; ++i)
        if (master[i] >= SW_ALPHABET) return fail(SW_E_INVALID, "master residue code out of range (use sw_encode)");
    for (int32_t k = 0; k < n; ++k)
        if (subject_of(mutable_db(db), ids[k]) < 0) return fail(SW_E_INVALID, "id not in the database");
    HIPCHECK(hipSetDevice(h->device));
    const size_t bytes = (static_cast<size_t>(n) + 1) * static_cast<size_t>(qlen);
    HIPCHECK(swk::dev_alloc(rows, std::max<size_t>(bytes, 1)));
    if (qlen > 0) {
        if (master) HIPCHECK(hipMemcpyAsync(rows.get(), master, qlen, hipMemcpyHostToDevice, h->stream.get()));
        else HIPCHECK(hipMemsetAsync(rows.get(), SW_MSA_NONE, qlen, h->stream.get()));
    }
    std::vector<sw_alignment> local(al ? 0 : static_cast<size_t>(n));
    if (int rc = align_impl(h, db, pssm_src(p, go, ge), ids, n, al ? al : local.data(), nullptr, 0, rows.get() + qlen))
        return rc;
    HIPCHECK(hipStreamSynchronize(h->stream.get()));  // (n == 0: the master's upload)
    return SW_OK;
}

// Step 2: the tables of rows[nrows][qlen] (device), the wanted ones into host memory.
int tables_of(sw_handle* h, const uint8_t* rows, int32_t nrows, int32_t qlen, uint32_t* cnt, uint64_t* weight,
              uint64_t* wsum) {
    if (qlen == 0) {  // no column: every row's coverage is 0
        if (weight) std::fill(weight, weight + nrows, uint64_t{0});
        return SW_OK;
    }
    const size_t cells = static_cast<size_t>(qlen) * SW_PROFILE_CODES;
    DevPtr<uint64_t> d64;  // wsum, then weight
    DevPtr<uint32_t> d32;  // cnt, then term
    HIPCHECK(swk::dev_alloc(d64, (cells + static_cast<size_t>(nrows)) * sizeof(uint64_t)));
    HIPCHECK(swk::dev_alloc(d32, 2 * cells * sizeof(uint32_t)));
    swk::MsaArgs a{};
    a.rows = rows;
    a.nrows = nrows;
    a.qlen = qlen;
    a.cnt = d32.get();
    a.term = d32.get() + cells;  // (aliases into d32 / d64)
    a.wsum = d64.get();
    a.weight = d64.get() + cells;
    hipStream_t const s = h->stream.get();
    HIPCHECK(swk::launch_msa_tables(a, s));
    h->launches += 3;
    if (cnt) HIPCHECK(hipMemcpyAsync(cnt, a.cnt, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (weight) HIPCHECK(hipMemcpyAsync(weight, a.weight, static_cast<size_t>(nrows) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (wsum) HIPCHECK(hipMemcpyAsync(wsum, a.wsum, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return check_fault(h);
}

int profile_counts(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t go, int32_t ge, const uint8_t* master,
                   const int32_t* ids, int32_t n, uint32_t* cnt, uint64_t* weight, uint64_t* wsum) {
    DevPtr<uint8_t> rows;
    if (int rc = build_rows(h, db, p, go, ge, master, ids, n, rows, nullptr)) return rc;
    return tables_of(h, rows.get(), n + 1, p->qlen, cnt, weight, wsum);
}

int refine(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t go, int32_t ge, const uint8_t* master,
           const int8_t* mat, double pseudo, const int32_t* ids, int32_t n, sw_pssm** out) {
    const size_t cells = static_cast<size_t>(p->qlen) * SW_PROFILE_CODES;
    std::vector<uint32_t> cnt(cells);
    std::vector<uint64_t> wsum(cells);
    if (int rc = profile_counts(h, db, p, go, ge, master, ids, n, cnt.data(), nullptr, wsum.data())) return rc;
    std::vector<int8_t> rows(static_cast<size_t>(p->qlen) * SW_ALPHABET);
    pssm_table(p, rows.data());
    if (!swprofile::pssm_from_counts(cnt.data(), wsum.data(), p->qlen, rows.data(), mat, pseudo, rows.data()))
        return fail(SW_E_UNSUPPORTED, "the matrix has no lambda (expected score >= 0, or no positive entry)");
    return sw_pssm_create(h, rows.data(), p->qlen, out);
}

// A PSSM the loop owns until it hands it out.
struct PssmGuard {
    sw_pssm* p = nullptr;
    ~PssmGuard() { sw_pssm_free(p); }
    void reset(sw_pssm* q) { sw_pssm_free(p); p = q; }
    sw_pssm* release() { sw_pssm* q = p; p = nullptr; return q; }
};

// One round's device state behind the handle's score row: the k keys, the
// count, the calibration table, the gathered rows (as sw_search.cpp's ranked_keys).
struct RoundBufs {
    int32_t* scores;
    int64_t* keys;
    uint32_t* count;
    uint32_t* hist;
    int32_t* rows;
};
int round_bufs(sw_handle* h, const sw_db* db, RoundBufs* b) {
    const int64_t rs = round_up(static_cast<int64_t>(db->max_id) + 1, 2);
    if (int rc = ensure_scores(h, static_cast<size_t>(rs) + 2 * kMaxHits + 2 + swcalib::kCells + 4 * kMaxHits)) return rc;
    b->scores = h->d_scores.get();
    b->keys = reinterpret_cast<int64_t*>(b->scores + rs);
    b->count = reinterpret_cast<uint32_t*>(b->keys + kMaxHits);
    b->hist = b->count + 2;
    b->rows = reinterpret_cast<int32_t*>(b->hist + swcalib::kCells);
    return SW_OK;
}

// The scan of p and its calibration (one synchronisation); the scores stay in b.scores.
int scan_round(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t go, int32_t ge, const RoundBufs& b,
               sw_calib* calib) {
    if (db->n == 0) {  // the calibration of an empty table
        const std::vector<uint32_t> zero(swcalib::kCells, 0);
        calib_of(db, zero.data(), p->qlen, calib);
        return SW_OK;
    }
    uint32_t* hist = nullptr;  // (pinned)
    if (int rc = ensure_hist_host(h, 1, &hist)) return rc;
    hipStream_t const s = h->stream.get();
    if (int rc = scan_impl(h, db, pssm_src(p, go, ge), b.scores, false, nullptr, b.hist)) return rc;
    HIPCHECK(hipMemcpyAsync(hist, b.hist, swcalib::kCells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (int rc = check_fault(h)) return rc;
    calib_of(db, hist, p->qlen, calib);
    return SW_OK;
}

// The key pass, selection and gather over b.scores under (k, max_evalue): the
// selected rows {id, score, subject length, 0} and the count that passed.
int select_round(sw_handle* h, const sw_db* db, const sw_calib& calib, const RoundBufs& b, int32_t k, double max_evalue,
                 std::vector<int32_t>* rows, int64_t* n_pass) {
    rows->clear();
    *n_pass = 0;
    if (db->n == 0) return SW_OK;
    int64_t r_min = 0;
    if (!swcalib::rank_min(calib, max_evalue, &r_min)) return fail(SW_E_INVALID, "an E-value bound must be > 0");
    std::vector<int32_t> adj(static_cast<size_t>(db->max_len) + 1);  // (alive until the synchronisation below)
    swcalib::rank_table(calib, db->max_len, adj.data());
    if (int rc = sig_topk_enqueue(h, mutable_db(db), b.scores, adj.data(), db->max_len, r_min, k, b.keys, b.count, b.rows))
        return rc;
    uint32_t count = 0;
    std::vector<int32_t> got(static_cast<size_t>(k) * 4);
    hipStream_t const s = h->stream.get();
    HIPCHECK(hipMemcpyAsync(&count, b.count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(got.data(), b.rows, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (int rc = check_fault(h)) return rc;
    *n_pass = count;
    got.resize(static_cast<size_t>(std::min<int64_t>(k, count)) * 4);
    rows->swap(got);
    return SW_OK;
}

}  // namespace

// ===========================================================================
extern "C" {

int sw_pssm_rows(const sw_pssm* p, int8_t* rows) {
    if (!p || (p->qlen > 0 && !rows)) return fail(SW_E_INVALID, "null argument");
    pssm_table(p, rows);
    return SW_OK;
}

int sw_msa_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                const uint8_t* master, const int32_t* ids, int32_t n, uint8_t* msa_host, sw_alignment* al) {
    if (!msa_host) return fail(SW_E_INVALID, "null argument");
    DevPtr<uint8_t> rows;
    if (int rc = build_rows(h, db, p, gap_open, gap_extend, master, ids, n, rows, al)) return rc;
    const size_t bytes = (static_cast<size_t>(n) + 1) * static_cast<size_t>(p->qlen);
    if (bytes) HIPCHECK(hipMemcpy(msa_host, rows.get(), bytes, hipMemcpyDeviceToHost));
    return check_fault(h);
}

int sw_profile_counts(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                      const uint8_t* master, const int32_t* ids, int32_t n, uint32_t* cnt, uint64_t* weight,
                      uint64_t* wsum) {
    return profile_counts(h, db, p, gap_open, gap_extend, master, ids, n, cnt, weight, wsum);
}

int sw_profile_counts_msa(sw_handle* h, const uint8_t* msa_host, int32_t nrows, int32_t qlen, uint32_t* cnt,
                          uint64_t* weight, uint64_t* wsum) {
    if (!h || nrows < 1 || nrows > kMaxHits + 1 || qlen < 0 || (qlen > 0 && !msa_host))
        return fail(SW_E_INVALID, "bad argument (1 <= nrows <= 4097)");
    if (int rc = check_fault(h)) return rc;
    HIPCHECK(hipSetDevice(h->device));
    DevPtr<uint8_t> rows;
    const size_t bytes = static_cast<size_t>(nrows) * static_cast<size_t>(qlen);
    if (bytes) {
        HIPCHECK(swk::dev_alloc(rows, bytes));
        HIPCHECK(hipMemcpyAsync(rows.get(), msa_host, bytes, hipMemcpyHostToDevice, h->stream.get()));
    }
    return tables_of(h, rows.get(), nrows, qlen, cnt, weight, wsum);
}

int sw_matrix_lambda(const int8_t* matrix, double* lambda) {
    if (!lambda) return fail(SW_E_INVALID, "null argument");
    const int8_t* mat = nullptr;
    if (int rc = matrix_of(matrix, &mat)) return rc;
    if (!swprofile::matrix_lambda(mat, lambda))
        return fail(SW_E_UNSUPPORTED, "the matrix has no lambda (expected score >= 0, or no positive entry)");
    return SW_OK;
}

int sw_pssm_from_counts(const uint32_t* cnt, const uint64_t* wsum, int32_t qlen, const int8_t* prior_rows,
                        const int8_t* matrix, double pseudo, int8_t* rows_out) {
    if (qlen < 0 || (qlen > 0 && (!cnt || !wsum || !prior_rows || !rows_out))) return fail(SW_E_INVALID, "null argument");
    if (!pseudo_ok(pseudo)) return fail(SW_E_INVALID, "pseudo must be in (0, 1000]");
    const int8_t* mat = nullptr;
    if (int rc = matrix_of(matrix, &mat)) return rc;
    if (!swprofile::pssm_from_counts(cnt, wsum, qlen, prior_rows, mat, pseudo, rows_out))
        return fail(SW_E_UNSUPPORTED, "the matrix has no lambda (expected score >= 0, or no positive entry)");
    return SW_OK;
}

int sw_pssm_refine(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                   const uint8_t* master, const int8_t* matrix, double pseudo, const int32_t* ids, int32_t n,
                   sw_pssm** out) {
    if (!out) return fail(SW_E_INVALID, "null argument");
    *out = nullptr;
    if (!pseudo_ok(pseudo)) return fail(SW_E_INVALID, "pseudo must be in (0, 1000]");
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    const int8_t* mat = nullptr;
    if (int rc = matrix_of(matrix, &mat)) return rc;
    return refine(h, db, p, gap_open, gap_extend, master, mat, pseudo, ids, n, out);
}

int sw_search_iter(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                   int32_t rounds, double inclusion_evalue, int32_t include_max, double pseudo, int32_t k,
                   double max_evalue, int32_t* ids, int32_t* scores, sw_sig* sig, int32_t* nhits, int64_t* n_pass,
                   sw_calib* calib, sw_iter_round* rounds_log, int32_t* rounds_run, int32_t* converged,
                   sw_pssm** final_pssm) {
    if (final_pssm) *final_pssm = nullptr;
    if (!h || !db || qlen < 0 || (qlen > 0 && !query) || !ids || !scores || !sig || !nhits || !n_pass || !rounds_run ||
        !converged)
        return fail(SW_E_INVALID, "null argument");
    *nhits = 0, *n_pass = 0, *rounds_run = 0, *converged = 0;
    if (rounds < 1 || include_max < 1 || include_max > kMaxHits || k < 1 || k > 4096)
        return fail(SW_E_INVALID, "bad argument (rounds >= 1, 1 <= include_max, k <= 4096)");
    if (!(inclusion_evalue > 0) || !(max_evalue > 0)) return fail(SW_E_INVALID, "an E-value bound must be > 0");
    if (!pseudo_ok(pseudo)) return fail(SW_E_INVALID, "pseudo must be in (0, 1000]");
    const int8_t* mat = nullptr;
    int go, ge, rc;
    if ((rc = check_scoring(sc, &mat, &go, &ge))) return rc;
    for (int32_t i = 0; i < qlen; ++i)
        if (query[i] >= SW_ALPHABET) return fail(SW_E_INVALID, "query residue code out of range (use sw_encode)");
    double lambda;
    if (rounds > 1 && !swprofile::matrix_lambda(mat, &lambda))
        return fail(SW_E_UNSUPPORTED, "the matrix has no lambda (expected score >= 0, or no positive entry)");
    if (db->h != h) return fail(SW_E_INVALID, "the database belongs to another handle");
    HIPCHECK(hipSetDevice(h->device));

    // P_1: the table the query stands for under the matrix
    std::vector<int8_t> rows(static_cast<size_t>(qlen) * SW_ALPHABET);
    for (int32_t i = 0; i < qlen; ++i) std::memcpy(&rows[static_cast<size_t>(i) * SW_ALPHABET], mat + SW_ALPHABET * query[i], SW_ALPHABET);
    PssmGuard cur;
    if ((rc = sw_pssm_create(h, rows.data(), qlen, &cur.p))) return rc;
    if ((rc = check_pssm(h, cur.p, go, ge))) return rc;

    RoundBufs b{};
    std::vector<int32_t> sel, prev, inc;
    sw_calib cal{};
    for (int32_t t = 1;; ++t) {
        if ((rc = round_bufs(h, db, &b))) return rc;
        if ((rc = scan_round(h, db, cur.p, go, ge, b, &cal))) return rc;
        int64_t pass = 0;
        if ((rc = select_round(h, db, cal, b, include_max, inclusion_evalue, &sel, &pass))) return rc;
        inc.clear();
        for (size_t i = 0; i < sel.size(); i += 4) inc.push_back(sel[i]);
        std::vector<int32_t> sorted = inc;
        std::sort(sorted.begin(), sorted.end());
        std::vector<int32_t> diff;
        std::set_difference(sorted.begin(), sorted.end(), prev.begin(), prev.end(), std::back_inserter(diff));
        const int32_t added = static_cast<int32_t>(diff.size());
        diff.clear();
        std::set_difference(prev.begin(), prev.end(), sorted.begin(), sorted.end(), std::back_inserter(diff));
        const int32_t dropped = static_cast<int32_t>(diff.size());
        if (rounds_log) rounds_log[t - 1] = sw_iter_round{static_cast<int32_t>(inc.size()), added, dropped, 0, cal};
        *rounds_run = t;
        const bool same = t > 1 && added == 0 && dropped == 0;
        prev.swap(sorted);
        if (same) *converged = 1;
        if (same || t == rounds) break;
        sw_pssm* next = nullptr;
        if ((rc = refine(h, db, cur.p, go, ge, query, mat, pseudo, inc.data(), static_cast<int32_t>(inc.size()), &next)))
            return rc;
        cur.reset(next);
    }
    // the report: a second key pass and selection over the last round's scores
    int64_t pass = 0;
    if ((rc = select_round(h, db, cal, b, k, max_evalue, &sel, &pass))) return rc;
    const int32_t m = static_cast<int32_t>(sel.size() / 4);
    for (int32_t i = 0; i < m; ++i) {
        ids[i] = sel[4 * i];
        scores[i] = sel[4 * i + 1];
        swcalib::significance(cal, sel[4 * i + 1], sel[4 * i + 2], &sig[i]);
    }
    *nhits = m;
    *n_pass = pass;
    if (calib) *calib = cal;
    if (final_pssm) *final_pssm = cur.release();
    return SW_OK;
}

}  // extern "C"
