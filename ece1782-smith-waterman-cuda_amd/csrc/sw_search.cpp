// sw_search.cpp — what the host driver (sw_driver.h) runs on top of a scan
// (sw_capi.cpp scan_impl): the synchronous forms into host memory, the
// rankings (top-K), the hit table, the calibration and significance, the
// traceback, the position-specific matrices, and the batches of all of them.
// The single-query entry points are the batch routines with one query.
#include <algorithm>
#include <new>
#include <numeric>

#include "sw_calib.h"
#include "sw_dbfile.h"
#include "sw_driver.h"

using namespace swd;

namespace swd {

int ensure_scores(sw_handle* h, size_t n) {
    if (n > h->scores_cap) {
        h->scores_cap = 0;
        const size_t cap = std::max<size_t>(n, 1024);
        HIPCHECK(swk::dev_alloc(h->d_scores, cap * 4));  // the old one released first: ~1 GiB (sw_scan_batch)
        h->scores_cap = cap;
    }
    return SW_OK;
}

}  // namespace swd

namespace {

// sw_scan / sw_scan_pssm: the synchronous scan into host memory.
int scan_host(sw_handle* h, const sw_db* db, const QuerySrc& src, int32_t* scores_host) {
    if (!h || !db || !scores_host) return fail(SW_E_INVALID, "null argument");
    const size_t n = static_cast<size_t>(db->max_id + 1);
    if (n == 0) return SW_OK;
    int rc;
    HIPCHECK(hipSetDevice(h->device));
    if ((rc = ensure_scores(h, n))) return rc;
    // slots that no subject maps to read 0
    HIPCHECK(hipMemsetAsync(h->d_scores.get(), 0, n * 4, h->stream.get()));
    if ((rc = scan_impl(h, db, src, h->d_scores.get()))) return rc;
    HIPCHECK(hipMemcpyAsync(scores_host, h->d_scores.get(), n * 4, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    return check_fault(h);
}

// The scans of srcs[0 .. nq) back to back on the handle's stream, each with
// its ranking (RankReq: the top-K follows every stage that writes that
// query's scores, its rescue tail included, and the next scan's writes follow
// it in stream order), into keys[nq][k] behind ONE score row; one copy and
// one synchronisation end the call.
// hist_host (nullable, [nq][128][512]): every query's calibration table too
// (sw_calib.h), behind the keys in device memory, in the same copy sequence
// and synchronisation.
int scan_topk_host(sw_handle* h, const sw_db* cdb, const QuerySrc* srcs, int32_t nq, int32_t k, int64_t* keys_host,
                   uint32_t* hist_host = nullptr) {
    sw_db* db = mutable_db(cdb);
    if (!h || !db || k <= 0 || k > 4096 || (nq > 0 && !keys_host)) return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (nq == 0) return SW_OK;
    const size_t nkeys = static_cast<size_t>(nq) * static_cast<size_t>(k);
    const size_t ntab = hist_host ? static_cast<size_t>(nq) * swcalib::kCells : 0;
    if (db->n == 0) {
        for (size_t i = 0; i < nkeys; ++i) keys_host[i] = INT64_MIN;
        if (hist_host) std::memset(hist_host, 0, ntab * sizeof(uint32_t));
        return SW_OK;
    }
    int rc;
    HIPCHECK(hipSetDevice(h->device));
    const size_t slots = static_cast<size_t>(db->max_id + 1);
    // the score row, then the nq x k keys, then the nq tables
    if ((rc = ensure_scores(h, slots + 2 * nkeys + 2 + ntab))) return rc;
    int64_t* keys_dev = reinterpret_cast<int64_t*>(h->d_scores.get() + round_up(static_cast<int64_t>(slots), 2));
    uint32_t* hist_dev = hist_host ? reinterpret_cast<uint32_t*>(keys_dev + nkeys) : nullptr;
    for (int32_t q = 0; q < nq; ++q) {
        // the ranking runs over the result ids of the subjects (rank_after)
        const RankReq rq{k, nullptr, 0, keys_dev + static_cast<size_t>(q) * k};
        if ((rc = scan_impl(h, db, srcs[q], h->d_scores.get(), false, &rq,
                            hist_dev ? hist_dev + static_cast<size_t>(q) * swcalib::kCells : nullptr)))
            return rc;
    }
    HIPCHECK(hipMemcpyAsync(keys_host, keys_dev, nkeys * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream.get()));
    if (hist_host)
        HIPCHECK(hipMemcpyAsync(hist_host, hist_dev, ntab * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    return check_fault(h);
}

// The queries of a batch as scan sources.
std::vector<QuerySrc> batch_srcs(const uint8_t* queries, const int64_t* qoffsets, int32_t nq, const sw_scoring* sc) {
    std::vector<QuerySrc> srcs(static_cast<size_t>(std::max(nq, 0)));
    for (int32_t q = 0; q < nq; ++q)
        srcs[q] = seq_src(queries + qoffsets[q], static_cast<int32_t>(qoffsets[q + 1] - qoffsets[q]), sc);
    return srcs;
}

int topk_impl(sw_handle* h, const int32_t* scores, const int64_t* keys, int64_t n, int64_t id_base,
              const int32_t* ids, int32_t k, int64_t* out) {
    if (!h || !out || n < 0 || k <= 0 || k > 4096 || (n > 0 && !scores && !keys))
        return fail(SW_E_INVALID, "bad top-k arguments (1 <= k <= 4096)");
    if (id_base < 0 || id_base + n > (int64_t(1) << 31)) return fail(SW_E_INVALID, "ids must fit in 31 bits");
    HIPCHECK(hipSetDevice(h->device));
    int rc;
    if ((rc = check_fault(h))) return rc;
    if ((rc = ensure_topk_work(h, swk::topk_workspace_bytes(n, k)))) return rc;
    swk::TopkSrc src{};
    src.scores = keys ? nullptr : scores;
    src.keys = keys;
    src.gid = ids;
    src.id_base = id_base;
    HIPCHECK(swk::launch_topk(src, n, k, out, h->d_topk_work.get(), h->stream.get()));
    return SW_OK;
}

}  // namespace

namespace swd {

// sw_align / sw_align_pssm: one traceback path; the forms differ in what is
// uploaded (the codes and the matrix, or nothing: the table is resident) and
// in the kernel's score functor (sw_align.hip).  msa_dev (nullable, device
// [n][qlen]): every hit's query-anchored row too (sw_refine.cpp).
int align_impl(sw_handle* h, const sw_db* cdb, const QuerySrc& src, const int32_t* ids, int32_t n,
               sw_alignment* out, char* ops, int64_t ops_stride, uint8_t* msa_dev) {
    sw_db* db = mutable_db(cdb);
    const uint8_t* query = src.codes;
    const int32_t qlen = src.qlen;
    if (!h || !db || n < 0 || qlen < 0 || (!src.pssm && qlen > 0 && !query) || (n > 0 && (!ids || !out)) ||
        (ops && ops_stride <= 0))
        return fail(SW_E_INVALID, "null argument");
    const int8_t* mat = nullptr;
    int go = src.go, ge = src.ge, rc;
    if (!src.pssm && (rc = check_scoring(src.sc, &mat, &go, &ge))) return rc;
    for (int32_t i = 0; i < qlen && !src.pssm; ++i)
        if (query[i] >= SW_ALPHABET) return fail(SW_E_INVALID, "query residue code out of range (use sw_encode)");
    std::vector<int64_t> sidx(n);
    for (int32_t k = 0; k < n; ++k)
        if ((sidx[k] = subject_of(db, ids[k])) < 0) return fail(SW_E_INVALID, "sw_align: id not in the database");
    std::memset(out, 0, sizeof(sw_alignment) * static_cast<size_t>(n));
    if (n == 0 || qlen == 0) return SW_OK;
    HIPCHECK(hipSetDevice(h->device));
    auto slen_of = [&](int64_t k) { return db->h_offsets[k + 1] - db->h_offsets[k]; };
    // groups of hits whose direction arrays fit the budget (swplan::align_groups)
    const int64_t W1 = static_cast<int64_t>(qlen) + 1;
    std::vector<int64_t> slens(static_cast<size_t>(n));
    for (int32_t k = 0; k < n; ++k) slens[k] = slen_of(sidx[k]);
    int32_t k0 = 0;
    for (const int64_t end : swplan::align_groups(qlen, slens.data(), n)) {
        const int32_t k1 = static_cast<int32_t>(end);
        int64_t res = 0;
        for (int32_t k = k0; k < k1; ++k) res += slens[k];
        const int32_t m = k1 - k0;
        std::vector<uint8_t> hsub(static_cast<size_t>(std::max<int64_t>(res, 1)));
        std::vector<int64_t> hoff(m + 1, 0), hdoff(m, 0);
        int64_t dacc = 0;
        for (int32_t k = 0; k < m; ++k) {
            const int64_t src = sidx[k0 + k], L = slen_of(src);
            subject_residues(db, src, hsub.data() + hoff[k]);
            hoff[k + 1] = hoff[k] + L;
            hdoff[k] = dacc;
            dacc += swplan::align_dirs_bytes(qlen, L);
        }
        std::vector<int32_t> hout(static_cast<size_t>(m) * 6);
        // this group's buffers (qlen, m >= 1: no empty one), released after the synchronise below
        DevPtr<uint8_t> dq, dsub, ddir;
        DevPtr<int64_t> doff, ddoff;
        DevPtr<int8_t> dmat;
        DevPtr<int32_t> dh, dout;
        DevPtr<char> dops;
        if (!src.pssm) HIPCHECK(swk::dev_alloc(dq, qlen));
        HIPCHECK(swk::dev_alloc(dsub, hsub.size()));
        HIPCHECK(swk::dev_alloc(doff, (m + 1) * sizeof(int64_t)));
        HIPCHECK(swk::dev_alloc(ddoff, m * sizeof(int64_t)));
        if (!src.pssm) HIPCHECK(swk::dev_alloc(dmat, 625));
        HIPCHECK(swk::dev_alloc(ddir, static_cast<size_t>(dacc)));
        // H: three diagonals; affine also two of E and two of F
        HIPCHECK(swk::dev_alloc(dh, static_cast<size_t>(m) * (go != ge ? 7 : 3) * W1 * sizeof(int32_t)));
        HIPCHECK(swk::dev_alloc(dout, static_cast<size_t>(m) * 6 * sizeof(int32_t)));
        if (ops) HIPCHECK(swk::dev_alloc(dops, static_cast<size_t>(m) * ops_stride));
        hipStream_t const s = h->stream.get();
        if (!src.pssm) HIPCHECK(hipMemcpyAsync(dq.get(), query, qlen, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(dsub.get(), hsub.data(), hsub.size(), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(doff.get(), hoff.data(), (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(ddoff.get(), hdoff.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (!src.pssm) HIPCHECK(hipMemcpyAsync(dmat.get(), mat, 625, hipMemcpyHostToDevice, s));
        swk::AlignArgs a{};
        a.query = dq.get();
        a.qlen = qlen;
        a.subj = dsub.get();
        a.subj_off = doff.get();
        a.n = m;
        a.mat = dmat.get();
        a.pssm = src.pssm ? src.pssm->d.get() : nullptr;
        a.pssm_ld = src.pssm ? src.pssm->ld : 0;
        a.gap = go;
        a.gap_extend = ge;
        a.dirs = ddir.get();
        a.dirs_off = ddoff.get();
        a.hbuf = dh.get();
        a.out = dout.get();
        a.ops = dops.get();
        a.ops_stride = ops ? ops_stride : 0;
        a.msa = msa_dev ? msa_dev + static_cast<int64_t>(k0) * qlen : nullptr;
        HIPCHECK(swk::launch_align(a, s));
        HIPCHECK(hipMemcpyAsync(hout.data(), dout.get(), hout.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (ops)
            HIPCHECK(hipMemcpyAsync(ops + static_cast<int64_t>(k0) * ops_stride, dops.get(),
                                    static_cast<size_t>(m) * ops_stride, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        for (int32_t k = 0; k < m; ++k) {
            sw_alignment& o = out[k0 + k];
            if (slen_of(sidx[k0 + k]) == 0) continue;  // empty subject: all zero (as the oracle)
            o.score = hout[6 * k];
            o.q_begin = hout[6 * k + 1];
            o.q_end = hout[6 * k + 2];
            o.s_begin = hout[6 * k + 3];
            o.s_end = hout[6 * k + 4];
            o.ops_len = hout[6 * k + 5];
        }
        k0 = k1;
    }
    return SW_OK;
}

}  // namespace swd

namespace {

// The hit table (sw_hits.hip): the rows of the pairs (query qidx[k], result
// id ids[k]), k in [0, n), into out[k]; qidx null: every pair is query 0's
// (sw_hit_stats).  The queries are those of a batch.  What goes up, once: the
// queries, the matrix and one descriptor per hit (its query, where its subject
// is resident, its row); what comes down, once: the rows.  The hits launch in
// swplan::hits_order's order, longest wavefront first, in groups whose
// boundary rows fit the scratch budget; one synchronisation ends the call.
int hits_impl(sw_handle* h, const sw_db* cdb, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
              const sw_scoring* sc, const int32_t* qidx, const int32_t* ids, int64_t n, sw_hit* out) {
    sw_db* db = mutable_db(cdb);
    if (!h || !db || n < 0 || n >= (int64_t(1) << 31) || nq < 0 || (nq > 0 && !qoffsets) || (n > 0 && (!ids || !out)))
        return fail(SW_E_INVALID, "null argument");
    const int64_t qbase = nq > 0 ? qoffsets[0] : 0, qtotal = nq > 0 ? qoffsets[nq] - qbase : 0;
    if (qtotal > 0 && !queries) return fail(SW_E_INVALID, "null argument");
    const int8_t* mat = nullptr;
    int go, ge, rc;
    if ((rc = check_scoring(sc, &mat, &go, &ge))) return rc;
    for (int64_t i = 0; i < qtotal; ++i)
        if (queries[qbase + i] >= SW_ALPHABET) return fail(SW_E_INVALID, "query residue code out of range (use sw_encode)");
    for (int64_t k = 0; k < n; ++k) {
        const int32_t qi = qidx ? qidx[k] : 0;
        if (qi < 0 || qi >= nq) return fail(SW_E_INVALID, "sw_hit_stats_batch: query index outside [0, nq)");
    }
    // per pair, in the caller's order: the lengths, and the row as the host knows it
    std::vector<swk::HitDesc> hit(static_cast<size_t>(n));
    std::vector<int32_t> qlens(static_cast<size_t>(n));
    std::vector<int64_t> slens(static_cast<size_t>(n));
    int64_t work = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t subj = subject_of(db, ids[k]);
        if (subj < 0) return fail(SW_E_INVALID, "sw_hit_stats: id not in the database");
        const int32_t qi = qidx ? qidx[k] : 0;
        const swpack::Location loc = swpack::locate(position_of(db, subj), db->shape.nlong);
        qlens[k] = static_cast<int32_t>(qoffsets[qi + 1] - qoffsets[qi]);
        slens[k] = db->h_offsets[subj + 1] - db->h_offsets[subj];
        if (qlens[k] + slens[k] >= (int64_t(1) << 31)) return fail(SW_E_INVALID, "sw_hit_stats: qlen + subject length must be < 2^31");
        hit[k] = swk::HitDesc{ids[k], static_cast<int32_t>(slens[k]), static_cast<int32_t>(loc.slot), loc.lane, 0,
                              qoffsets[qi] - qbase, qlens[k], static_cast<int32_t>(k)};
        work += swplan::hits_cost(qlens[k], slens[k]);
    }
    for (int64_t k = 0; k < n; ++k) {
        std::memset(&out[k], 0, sizeof(sw_hit));
        out[k].id = ids[k];
        out[k].s_len = hit[k].slen;
    }
    if (work == 0) return SW_OK;  // no pair has a cell: every row is the zero row above
    HIPCHECK(hipSetDevice(h->device));
    // the launch order; then groups of hits, in that order, whose boundary
    // rows fit the scratch budget.  A group's rows start at column 0, and every
    // multi-chunk hit has its own (two queries may hit one subject).
    const std::vector<int64_t> order = swplan::hits_order(qlens.data(), slens.data(), n);
    std::vector<swk::HitDesc> desc(static_cast<size_t>(n));
    std::vector<int32_t> oq(static_cast<size_t>(n));
    std::vector<int64_t> os(static_cast<size_t>(n));
    for (int64_t k = 0; k < n; ++k) {
        desc[k] = hit[order[k]];
        oq[k] = qlens[order[k]];
        os[k] = slens[order[k]];
    }
    const std::vector<int64_t> ends = swplan::hits_groups(oq.data(), os.data(), n);
    int64_t cols_max = 0;
    int32_t qlen_max = 0;
    for (size_t g = 0, k = 0; g < ends.size(); ++g) {
        int64_t cols = 0;
        for (; k < static_cast<size_t>(ends[g]); ++k) {
            desc[k].scratch = cols;
            if (oq[k] > swk::kHitsChunkRows) cols += os[k];
            if (os[k] > 0) qlen_max = std::max(qlen_max, oq[k]);  // (an empty subject's workgroup returns at once)
        }
        cols_max = std::max(cols_max, cols);
    }
    // one allocation: the queries, the matrix, the descriptors, the rows (each 16-byte aligned)
    const size_t qbytes = static_cast<size_t>(round_up(qtotal, 16)), mbytes = 640;
    const size_t dbytes = static_cast<size_t>(round_up(static_cast<int64_t>(desc.size() * sizeof(swk::HitDesc)), 16));
    DevPtr<uint8_t> dq;
    DevPtr<int32_t> dbnd;
    HIPCHECK(swk::dev_alloc(dq, qbytes + mbytes + dbytes + static_cast<size_t>(n) * sizeof(sw_hit)));
    swk::HitDesc* const ddesc = reinterpret_cast<swk::HitDesc*>(dq.get() + qbytes + mbytes);  // (aliases into dq)
    sw_hit* const dout = reinterpret_cast<sw_hit*>(dq.get() + qbytes + mbytes + dbytes);
    const int64_t bnd_bytes = swplan::hits_scratch_bytes(qlen_max, cols_max);
    if (bnd_bytes) HIPCHECK(swk::dev_alloc(dbnd, static_cast<size_t>(bnd_bytes)));
    hipStream_t const s = h->stream.get();
    HIPCHECK(hipMemcpyAsync(dq.get(), queries + qbase, static_cast<size_t>(qtotal), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(dq.get() + qbytes, mat, 625, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ddesc, desc.data(), desc.size() * sizeof(swk::HitDesc), hipMemcpyHostToDevice, s));
    swk::HitArgs a{};
    a.query = dq.get();
    a.qlen_max = qlen_max;
    a.mat = reinterpret_cast<const int8_t*>(dq.get() + qbytes);
    a.gap_open = go;
    a.gap_extend = ge;
    a.res = db->lay.d_res.get();
    a.blk_off = db->lay.d_blk_off.get();
    a.lres = db->lay.d_lres.get();
    a.loff = db->lay.d_loff.get();
    a.bnd = dbnd.get();
    a.out = dout;  // a hit writes its own row (HitDesc::row): the caller's order
    int64_t k0 = 0;
    for (const int64_t k1 : ends) {  // in stream order: the groups share the scratch
        a.hits = ddesc + k0;
        a.n = static_cast<int32_t>(k1 - k0);
        HIPCHECK(swk::launch_hits(a, s));
        k0 = k1;
    }
    HIPCHECK(hipMemcpyAsync(out, dout, static_cast<size_t>(n) * sizeof(sw_hit), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return SW_OK;
}

// The batch's argument checks, shared by the batch calls below.
int check_batch_args(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq) {
    if (!h || !db || nq < 0 || (nq > 0 && !qoffsets)) return fail(SW_E_INVALID, "null argument");
    if (int rc = check_batch(qoffsets, nq)) return rc;
    if (nq > 0 && qoffsets[nq] > qoffsets[0] && !queries) return fail(SW_E_INVALID, "null argument");
    return SW_OK;
}

}  // namespace

namespace swd {

// The handle's pinned landing area holds at least n tables.
int ensure_hist_host(sw_handle* h, size_t n, uint32_t** out) {
    if (n > h->hist_cap) {
        HIPCHECK(hipSetDevice(h->device));
        HIPCHECK(hipStreamSynchronize(h->stream.get()));  // (a copy of an earlier call has long landed; be sure)
        h->hist_cap = 0;
        HIPCHECK(swk::host_alloc(h->h_hist, n * swcalib::kCells * sizeof(uint32_t), hipHostMallocDefault));
        h->hist_cap = n;
    }
    *out = h->h_hist.get();
    return SW_OK;
}

// A scan's calibration from its table (sw_calib.h): the fit, and the
// zero-length subjects the table does not hold.
void calib_of(const sw_db* db, const uint32_t* hist, int32_t qlen, sw_calib* out) {
    swcalib::fit(hist, qlen, out);
    out->n_skipped = db->n - out->n_db;
}

}  // namespace swd

namespace {

// What the four scan-and-hits entry points check first (*nhits starts at 0).
int check_hits_args(sw_handle* h, const sw_db* db, int32_t nq, int32_t k, sw_hit* out, int32_t* nhits, bool with_sig,
                    sw_sig* sig) {
    if (!h || !db || !nhits || k <= 0 || k > 4096 || (nq > 0 && (!out || (with_sig && !sig))))
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    *nhits = 0;
    return SW_OK;
}

// The scans of a batch with their rankings, then the hit-table rows of every
// query's min(k, n) best subjects in one launch sequence: two host
// synchronisations whatever nq is.  out is [nq][k] rows; sig (nullable,
// [nq][k]): the tables come down with the keys, for sig and calib (nullable, [nq]).
// The callers have checked their arguments (check_hits_args; the batch forms
// check_batch_args: a single query may be longer than a batch allows).
int scan_hits(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
              const sw_scoring* sc, int32_t k, sw_hit* out, int32_t* nhits, sw_sig* sig, sw_calib* calib) {
    const bool with_sig = sig != nullptr;
    int rc;
    // first synchronisation: every query's keys (and table)
    std::vector<int64_t> keys(static_cast<size_t>(std::max(nq, 0)) * static_cast<size_t>(k));
    uint32_t* hist = nullptr;  // (pinned: the tables come down in the keys' synchronisation)
    if (with_sig && nq > 0 && (rc = ensure_hist_host(h, static_cast<size_t>(nq), &hist))) return rc;
    if ((rc = scan_topk_host(h, db, batch_srcs(queries, qoffsets, nq, sc).data(), nq, k, keys.data(), hist))) return rc;
    const int32_t m = static_cast<int32_t>(std::min<int64_t>(k, db->n));
    // second: the rows of all nq x m pairs, one launch sequence
    const size_t np = static_cast<size_t>(nq) * static_cast<size_t>(m);
    std::vector<int32_t> qidx(np), ids(np);
    std::vector<sw_hit> rows(np);
    for (int32_t q = 0; q < nq; ++q)
        for (int32_t i = 0; i < m; ++i) {
            qidx[static_cast<size_t>(q) * m + i] = q;
            ids[static_cast<size_t>(q) * m + i] =
                static_cast<int32_t>(0x7fffffff - (keys[static_cast<size_t>(q) * k + i] & 0xffffffffll));
        }
    if ((rc = hits_impl(h, db, queries, qoffsets, nq, sc, qidx.data(), ids.data(), static_cast<int64_t>(np), rows.data())))
        return rc;
    for (int32_t q = 0; q < nq && m > 0; ++q)
        std::memcpy(out + static_cast<size_t>(q) * k, rows.data() + static_cast<size_t>(q) * m, static_cast<size_t>(m) * sizeof(sw_hit));
    for (int32_t q = 0; q < nq && with_sig; ++q) {
        sw_calib c;
        calib_of(db, hist + static_cast<size_t>(q) * swcalib::kCells,
                 static_cast<int32_t>(qoffsets[q + 1] - qoffsets[q]), &c);
        for (int32_t i = 0; i < m; ++i) {
            const sw_hit& r = rows[static_cast<size_t>(q) * m + i];
            swcalib::significance(c, r.score, r.s_len, &sig[static_cast<size_t>(q) * k + i]);
        }
        if (calib) calib[q] = c;
    }
    *nhits = m;
    return check_fault(h);
}

}  // namespace

namespace swd {

// ---- ranking by E-value (include/sw_amd.h; sw_sigkeys.hip) ---------------------
// sw_sig_topk_device's enqueue, on the handle's stream: the adjustment table
// goes up, the count is zeroed, every subject's key is written into the
// handle's workspace behind the top-K's own part, and the existing top-K
// selects over those n keys.  rows (nullable, device [k][4]): the gather too.
int sig_topk_enqueue(sw_handle* h, sw_db* db, const int32_t* scores_dev, const int32_t* adj_host, int32_t max_len,
                     int64_t r_min, int32_t k, int64_t* keys_out_dev, uint32_t* count_out_dev, int32_t* rows_dev) {
    const int64_t n = db->n;
    const size_t tw = static_cast<size_t>(round_up(static_cast<int64_t>(swk::topk_workspace_bytes(n, k)), 8));
    const size_t kbytes = static_cast<size_t>(n) * sizeof(int64_t);
    const size_t abytes = (static_cast<size_t>(max_len) + 1) * sizeof(int32_t);
    int rc;
    if ((rc = ensure_topk_work(h, tw + kbytes + abytes))) return rc;
    int64_t* const keys = h->d_topk_work.get() + tw / sizeof(int64_t);  // (aliases into the workspace)
    int32_t* const adj = reinterpret_cast<int32_t*>(keys + n);
    hipStream_t const s = h->stream.get();
    HIPCHECK(hipMemcpyAsync(adj, adj_host, abytes, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(count_out_dev, 0, sizeof(uint32_t), s));
    const int32_t *rid = nullptr, *slen = nullptr;
    if (n > 0) {
        if ((rc = subject_ids(db, &rid))) return rc;
        if ((rc = subject_lengths(db, &slen))) return rc;
    }
    HIPCHECK(swk::launch_sig_keys(scores_dev, rid, slen, adj, max_len, r_min, n, keys, count_out_dev, s));
    swk::TopkSrc src{};
    src.keys = keys;
    HIPCHECK(swk::launch_topk(src, n, k, keys_out_dev, h->d_topk_work.get(), s));
    h->launches += 2;
    if (rows_dev) {
        HIPCHECK(swk::launch_sig_gather(scores_dev, rid, slen, keys, n, keys_out_dev, k, rows_dev, s));
        ++h->launches;
    }
    return SW_OK;
}

}  // namespace swd

namespace {

// What the ranked forms bring down: per query k keys, the count of subjects
// that passed, the calibration, and (PSSM form) k gathered rows of 4 ints.
struct Ranked {
    std::vector<int64_t> keys;
    std::vector<uint32_t> count;
    std::vector<sw_calib> calib;
    std::vector<int32_t> rows;
};

// The scans of srcs[0 .. nq) ranked by E-value.  A query's fit precedes its
// ranking, so the batch keeps G score rows (swplan::ranked_groups) and runs
// groups of G queries: the scans and their tables, one synchronisation, the
// fits, then the G key passes and selections in stream order; one more
// synchronisation brings every query's keys and count down.
int ranked_keys(sw_handle* h, const sw_db* cdb, const QuerySrc* srcs, int32_t nq, int32_t k, double max_evalue,
                int64_t score_bytes, bool gather, Ranked& o) {
    sw_db* db = mutable_db(cdb);
    const size_t nkeys = static_cast<size_t>(nq) * static_cast<size_t>(k);
    o.keys.assign(nkeys, INT64_MIN);
    o.count.assign(static_cast<size_t>(nq), 0);
    o.calib.assign(static_cast<size_t>(nq), sw_calib{});
    o.rows.assign(gather ? nkeys * 4 : 0, 0);
    if (nq == 0) return SW_OK;
    if (db->n == 0) {  // the calibration of an empty table
        const std::vector<uint32_t> zero(swcalib::kCells, 0);
        for (int32_t q = 0; q < nq; ++q) calib_of(db, zero.data(), srcs[q].qlen, &o.calib[q]);
        return SW_OK;
    }
    if (db->h != h) return fail(SW_E_INVALID, "the database belongs to another handle");
    int rc;
    HIPCHECK(hipSetDevice(h->device));
    const int64_t slots = static_cast<int64_t>(db->max_id) + 1, rs = round_up(slots, 2);
    const int32_t G = swplan::ranked_groups(nq, slots, score_bytes);
    // the G score rows, then the keys, the counts, the G tables, the gathered rows
    const size_t ncnt = static_cast<size_t>(round_up(nq, 2));
    const size_t ntab = static_cast<size_t>(G) * swcalib::kCells;
    if ((rc = ensure_scores(h, static_cast<size_t>(G) * rs + 2 * nkeys + ncnt + ntab + o.rows.size()))) return rc;
    int64_t* const keys_dev = reinterpret_cast<int64_t*>(h->d_scores.get() + static_cast<size_t>(G) * rs);
    uint32_t* const cnt_dev = reinterpret_cast<uint32_t*>(keys_dev + nkeys);
    uint32_t* const hist_dev = cnt_dev + ncnt;
    int32_t* const rows_dev = gather ? reinterpret_cast<int32_t*>(hist_dev + ntab) : nullptr;
    uint32_t* hist = nullptr;  // (pinned)
    if ((rc = ensure_hist_host(h, static_cast<size_t>(G), &hist))) return rc;
    hipStream_t const s = h->stream.get();
    // every query's adjustment table stays alive until the last synchronisation (its upload's source)
    std::vector<std::vector<int32_t>> adj(static_cast<size_t>(nq));
    for (int32_t g0 = 0; g0 < nq; g0 += G) {
        const int32_t m = std::min(G, nq - g0);
        for (int32_t j = 0; j < m; ++j)
            if ((rc = scan_impl(h, db, srcs[g0 + j], h->d_scores.get() + static_cast<size_t>(j) * rs, false, nullptr,
                                hist_dev + static_cast<size_t>(j) * swcalib::kCells)))
                return rc;
        HIPCHECK(hipMemcpyAsync(hist, hist_dev, static_cast<size_t>(m) * swcalib::kCells * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        if ((rc = check_fault(h))) return rc;
        for (int32_t j = 0; j < m; ++j) {
            const int32_t q = g0 + j;
            calib_of(db, hist + static_cast<size_t>(j) * swcalib::kCells, srcs[q].qlen, &o.calib[q]);
            int64_t r_min = 0;
            if (!swcalib::rank_min(o.calib[q], max_evalue, &r_min)) return fail(SW_E_INVALID, "max_evalue must be > 0");
            adj[q].resize(static_cast<size_t>(db->max_len) + 1);
            swcalib::rank_table(o.calib[q], db->max_len, adj[q].data());
            if ((rc = sig_topk_enqueue(h, db, h->d_scores.get() + static_cast<size_t>(j) * rs, adj[q].data(), db->max_len,
                                       r_min, k, keys_dev + static_cast<size_t>(q) * k, cnt_dev + q,
                                       rows_dev ? rows_dev + static_cast<size_t>(q) * k * 4 : nullptr)))
                return rc;
        }
    }
    HIPCHECK(hipMemcpyAsync(o.keys.data(), keys_dev, nkeys * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(o.count.data(), cnt_dev, static_cast<size_t>(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (gather) HIPCHECK(hipMemcpyAsync(o.rows.data(), rows_dev, o.rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    return check_fault(h);
}

// sw_scan_hits_ranked and its batch form: ranked_keys, then the hit-table
// rows of every query's min(k, n_pass) selected ids in one launch sequence.
int scan_hits_ranked(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                     const sw_scoring* sc, int32_t k, double max_evalue, int64_t score_bytes, sw_hit* out, sw_sig* sig,
                     int32_t* nhits, int64_t* n_pass, sw_calib* calib) {
    Ranked r;
    int rc;
    if ((rc = ranked_keys(h, db, batch_srcs(queries, qoffsets, nq, sc).data(), nq, k, max_evalue, score_bytes, false, r)))
        return rc;
    std::vector<int32_t> qidx, ids;
    std::vector<size_t> first(static_cast<size_t>(nq) + 1, 0);
    for (int32_t q = 0; q < nq; ++q) {
        const int32_t m = static_cast<int32_t>(std::min<int64_t>(k, r.count[q]));
        for (int32_t i = 0; i < m; ++i) {
            qidx.push_back(q);
            ids.push_back(swcalib::rank_key_id(r.keys[static_cast<size_t>(q) * k + i]));
        }
        first[q + 1] = ids.size();
    }
    std::vector<sw_hit> rows(ids.size());
    if ((rc = hits_impl(h, db, queries, qoffsets, nq, sc, qidx.data(), ids.data(), static_cast<int64_t>(ids.size()),
                        rows.data())))
        return rc;
    for (int32_t q = 0; q < nq; ++q) {
        const size_t m = first[q + 1] - first[q];
        for (size_t i = 0; i < m; ++i) {
            const sw_hit& row = rows[first[q] + i];
            out[static_cast<size_t>(q) * k + i] = row;
            swcalib::significance(r.calib[q], row.score, row.s_len, &sig[static_cast<size_t>(q) * k + i]);
        }
        nhits[q] = static_cast<int32_t>(m);
        n_pass[q] = r.count[q];
        if (calib) calib[q] = r.calib[q];
    }
    return check_fault(h);
}

// What the ranked entry points check first (nhits and n_pass start at 0).
int check_ranked_args(sw_handle* h, const sw_db* db, int32_t nq, int32_t k, double max_evalue, const void* out,
                      const sw_sig* sig, int32_t* nhits, int64_t* n_pass) {
    if (!h || !db || k <= 0 || k > 4096 || nq < 0 || (nq > 0 && (!nhits || !n_pass || !out || !sig)))
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (!(max_evalue > 0)) return fail(SW_E_INVALID, "max_evalue must be > 0 (+inf: no cutoff)");
    for (int32_t q = 0; q < nq; ++q) nhits[q] = 0, n_pass[q] = 0;
    return SW_OK;
}

}  // namespace

// ===========================================================================
extern "C" {

int sw_scan(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
            int32_t* scores_host) {
    return scan_host(h, db, seq_src(query, qlen, sc), scores_host);
}

int sw_scan_batch(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                  const sw_scoring* sc, int32_t* scores_host) {
    if (!h || !db || nq < 0 || (nq > 0 && (!qoffsets || !queries || !scores_host)))
        return fail(SW_E_INVALID, "null argument");
    int rc;
    if ((rc = check_batch(qoffsets, nq))) return rc;
    const size_t n = static_cast<size_t>(db->max_id + 1);
    if (n == 0 || nq == 0) return SW_OK;
    HIPCHECK(hipSetDevice(h->device));
    // chunks of queries whose score rows fit in ~1 GiB of device memory
    const int32_t chunk = static_cast<int32_t>(std::max<size_t>(1, std::min<size_t>(nq, (size_t(1) << 30) / (n * 4))));
    if ((rc = ensure_scores(h, chunk * n))) return rc;
    for (int32_t k0 = 0; k0 < nq; k0 += chunk) {
        const int32_t m = std::min(chunk, nq - k0);
        HIPCHECK(hipMemsetAsync(h->d_scores.get(), 0, m * n * 4, h->stream.get()));  // unmapped slots read 0
        if ((rc = sw_scan_batch_device(h, db, queries, qoffsets + k0, m, sc, h->d_scores.get()))) return rc;
        HIPCHECK(hipMemcpyAsync(scores_host + k0 * n, h->d_scores.get(), m * n * 4, hipMemcpyDeviceToHost,
                                h->stream.get()));
        HIPCHECK(hipStreamSynchronize(h->stream.get()));
        if ((rc = check_fault(h))) return rc;
    }
    return SW_OK;
}

// ---- rankings ---------------------------------------------------------------
int sw_topk(const int32_t* scores, int64_t n, int32_t k, int32_t* out_ids, int32_t* out_scores) {
    if ((!scores && n > 0) || k < 0 || (k > 0 && (!out_ids || !out_scores))) return fail(SW_E_INVALID, "null argument");
    const int64_t kk = std::min<int64_t>(k, n);
    std::vector<int32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    auto cmp = [&](int32_t a, int32_t b) { return scores[a] != scores[b] ? scores[a] > scores[b] : a < b; };
    std::partial_sort(idx.begin(), idx.begin() + kk, idx.end(), cmp);
    for (int64_t i = 0; i < kk; ++i) {
        out_ids[i] = idx[i];
        out_scores[i] = scores[idx[i]];
    }
    for (int64_t i = kk; i < k; ++i) {
        out_ids[i] = -1;
        out_scores[i] = 0;
    }
    return SW_OK;
}

int sw_topk_device(sw_handle* h, const int32_t* scores_dev, int64_t n, int64_t id_base, int32_t k,
                   int64_t* keys_out_dev) {
    return topk_impl(h, scores_dev, nullptr, n, id_base, nullptr, k, keys_out_dev);
}

int sw_topk_device_ids(sw_handle* h, const int32_t* scores_dev, int64_t n, const int32_t* ids_dev, int32_t k,
                       int64_t* keys_out_dev) {
    if (n > 0 && !ids_dev) return fail(SW_E_INVALID, "null id map");
    return topk_impl(h, scores_dev, nullptr, n, 0, ids_dev, k, keys_out_dev);
}

int sw_topk_keys_device(sw_handle* h, const int64_t* keys_dev, int64_t n, int32_t k, int64_t* keys_out_dev) {
    return topk_impl(h, nullptr, keys_dev, n, 0, nullptr, k, keys_out_dev);
}

int sw_scan_topk(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc, int32_t k,
                 int64_t* keys_host) {
    const QuerySrc src = seq_src(query, qlen, sc);
    return scan_topk_host(h, db, &src, 1, k, keys_host);
}

int sw_scan_batch_topk(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                       const sw_scoring* sc, int32_t k, int64_t* keys_host) {
    if (int rc = check_batch_args(h, db, queries, qoffsets, nq)) return rc;
    return scan_topk_host(h, db, batch_srcs(queries, qoffsets, nq, sc).data(), nq, k, keys_host);
}

// ---- the hit table ------------------------------------------------------------
int sw_hit_stats(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                 const int32_t* ids, int32_t n, sw_hit* out) {
    if (qlen < 0 || (qlen > 0 && !query)) return fail(SW_E_INVALID, "null argument");
    const int64_t offs[2] = {0, qlen};  // one query as a batch of one
    return hits_impl(h, db, query, offs, 1, sc, nullptr, ids, n, out);
}

int sw_hit_stats_batch(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                       const sw_scoring* sc, const int32_t* qidx, const int32_t* ids, int64_t n, sw_hit* out) {
    int rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    if (n < 0 || n >= (int64_t(1) << 31) || (n > 0 && (!qidx || !ids || !out)))
        return fail(SW_E_INVALID, "bad argument (0 <= n < 2^31)");
    if ((rc = hits_impl(h, db, queries, qoffsets, nq, sc, qidx, ids, n, out))) return rc;
    return check_fault(h);
}

int sw_scan_batch_hits(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                       const sw_scoring* sc, int32_t k, sw_hit* out, int32_t* nhits) {
    int rc;
    if ((rc = check_hits_args(h, db, nq, k, out, nhits, false, nullptr))) return rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    return scan_hits(h, db, queries, qoffsets, nq, sc, k, out, nhits, nullptr, nullptr);
}

int sw_scan_batch_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                           const sw_scoring* sc, int32_t k, sw_hit* out, sw_sig* sig, int32_t* nhits,
                           sw_calib* calib) {
    int rc;
    if ((rc = check_hits_args(h, db, nq, k, out, nhits, true, sig))) return rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    return scan_hits(h, db, queries, qoffsets, nq, sc, k, out, nhits, sig, calib);
}

int sw_scan_hits(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc, int32_t k,
                 sw_hit* out, int32_t* nhits) {
    if (int rc = check_hits_args(h, db, 1, k, out, nhits, false, nullptr)) return rc;
    const int64_t offs[2] = {0, qlen};
    return scan_hits(h, db, query, offs, 1, sc, k, out, nhits, nullptr, nullptr);
}

int sw_scan_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                     int32_t k, sw_hit* out, sw_sig* sig, int32_t* nhits, sw_calib* calib) {
    if (!sig) return fail(SW_E_INVALID, "null argument");
    if (int rc = check_hits_args(h, db, 1, k, out, nhits, true, sig)) return rc;
    const int64_t offs[2] = {0, qlen};
    return scan_hits(h, db, query, offs, 1, sc, k, out, nhits, sig, calib);
}

// ---- the calibration alone (sw_calib.h) -------------------------------------
int sw_score_hist_device(sw_handle* h, const sw_db* cdb, const int32_t* scores_dev, uint32_t* hist_dev) {
    sw_db* db = mutable_db(cdb);
    if (!h || !db || !hist_dev || (db->n > 0 && !scores_dev)) return fail(SW_E_INVALID, "null argument");
    if (db->h != h) return fail(SW_E_INVALID, "the database belongs to another handle");
    int rc;
    if ((rc = check_fault(h))) return rc;
    HIPCHECK(hipSetDevice(h->device));
    if (!db->lay.built && (rc = build_db(db))) return rc;
    return hist_after(h, db, scores_dev, hist_dev);
}

int sw_score_hist(sw_handle* h, const sw_db* db, const int32_t* scores_dev, uint32_t* hist_host) {
    if (!h || !hist_host) return fail(SW_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(h->device));
    if (!h->d_hist.get()) HIPCHECK(swk::dev_alloc(h->d_hist, swcalib::kCells * sizeof(uint32_t)));
    if (int rc = sw_score_hist_device(h, db, scores_dev, h->d_hist.get())) return rc;
    HIPCHECK(hipMemcpyAsync(hist_host, h->d_hist.get(), swcalib::kCells * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    return check_fault(h);
}

int sw_calib_fit(const uint32_t* hist, int32_t qlen, sw_calib* out) {
    if (!hist || !out || qlen < 0) return fail(SW_E_INVALID, "null argument");
    swcalib::fit(hist, qlen, out);
    return SW_OK;
}

int sw_calib_sig(const sw_calib* calib, int32_t score, int32_t slen, sw_sig* out) {
    if (!calib || !out) return fail(SW_E_INVALID, "null argument");
    if (calib->size != static_cast<int32_t>(sizeof(sw_calib)))
        return fail(SW_E_INVALID, "sw_calib.size is not this library's (use sw_calib_fit)");
    swcalib::significance(*calib, score, slen, out);
    return SW_OK;
}

// ---- ranking by E-value -------------------------------------------------------
static int check_calib(const sw_calib* calib) {
    if (!calib) return fail(SW_E_INVALID, "null argument");
    if (calib->size != static_cast<int32_t>(sizeof(sw_calib)))
        return fail(SW_E_INVALID, "sw_calib.size is not this library's (use sw_calib_fit)");
    return SW_OK;
}

int sw_sig_rank_table(const sw_calib* calib, int32_t max_len, int32_t* adj) {
    if (int rc = check_calib(calib)) return rc;
    if (!adj || max_len < 0) return fail(SW_E_INVALID, "null argument");
    swcalib::rank_table(*calib, max_len, adj);
    return SW_OK;
}

int sw_sig_rank_min(const sw_calib* calib, double max_evalue, int64_t* r_min) {
    if (int rc = check_calib(calib)) return rc;
    if (!r_min) return fail(SW_E_INVALID, "null argument");
    if (!swcalib::rank_min(*calib, max_evalue, r_min)) return fail(SW_E_INVALID, "max_evalue must be > 0 (+inf: no cutoff)");
    return SW_OK;
}

int sw_sig_topk_device(sw_handle* h, const sw_db* cdb, const int32_t* scores_dev, const int32_t* adj_host,
                       int32_t max_len, int64_t r_min, int32_t k, int64_t* keys_out_dev, uint32_t* count_out_dev) {
    sw_db* db = mutable_db(cdb);
    if (!h || !db || !adj_host || max_len < 0 || !keys_out_dev || !count_out_dev || k <= 0 || k > 4096 ||
        (db->n > 0 && !scores_dev))
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (db->h != h) return fail(SW_E_INVALID, "the database belongs to another handle");
    int rc;
    if ((rc = check_fault(h))) return rc;
    HIPCHECK(hipSetDevice(h->device));
    if (!db->lay.built && (rc = build_db(db))) return rc;
    return sig_topk_enqueue(h, db, scores_dev, adj_host, max_len, r_min, k, keys_out_dev, count_out_dev, nullptr);
}

int sw_scan_hits_ranked(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                        int32_t k, double max_evalue, sw_hit* out, sw_sig* sig, int32_t* nhits, int64_t* n_pass,
                        sw_calib* calib) {
    if (int rc = check_ranked_args(h, db, 1, k, max_evalue, out, sig, nhits, n_pass)) return rc;
    const int64_t offs[2] = {0, qlen};
    return scan_hits_ranked(h, db, query, offs, 1, sc, k, max_evalue, 0, out, sig, nhits, n_pass, calib);
}

int sw_scan_batch_hits_ranked(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                              const sw_scoring* sc, int32_t k, double max_evalue, int64_t score_bytes, sw_hit* out,
                              sw_sig* sig, int32_t* nhits, int64_t* n_pass, sw_calib* calib) {
    int rc;
    if ((rc = check_ranked_args(h, db, nq, k, max_evalue, out, sig, nhits, n_pass))) return rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    return scan_hits_ranked(h, db, queries, qoffsets, nq, sc, k, max_evalue, score_bytes, out, sig, nhits, n_pass, calib);
}

// ---- position-specific scoring matrices ----------------------------------
int sw_pssm_create(sw_handle* h, const int8_t* rows, int32_t qlen, sw_pssm** out) {
    if (!h || !out || qlen < 0 || (qlen > 0 && !rows)) return fail(SW_E_INVALID, "null argument");
    *out = nullptr;
    const int64_t n = static_cast<int64_t>(qlen) * SW_ALPHABET;
    for (int64_t k = 0; k < n; ++k)
        if (rows[k] < -100 || rows[k] > 100) return fail(SW_E_INVALID, "PSSM entries must be in -100..100");
    std::unique_ptr<sw_pssm> p(new (std::nothrow) sw_pssm);
    if (!p) return fail(SW_E_NOMEM, "out of host memory");
    p->h = h;
    p->qlen = qlen;
    p->ld = static_cast<int32_t>(round_up(std::max<int32_t>(qlen, 1), 64));
    p->hash = swdbfile::fnv1a(swdbfile::kFnvBasis, rows, static_cast<size_t>(n));
    p->max_entry = n ? -128 : 0;
    // the resident image: transposed, [code][ld] (swk::PssmProfileArgs)
    p->image.assign(static_cast<size_t>(SW_ALPHABET) * p->ld, 0);
    for (int32_t i = 0; i < qlen; ++i)
        for (int c = 0; c < SW_ALPHABET; ++c) {
            const int8_t v = rows[static_cast<int64_t>(i) * SW_ALPHABET + c];
            p->max_entry = std::max<int>(p->max_entry, v);
            p->image[static_cast<size_t>(c) * p->ld + i] = v;
        }
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(swk::dev_alloc(p->d, p->image.size()));
    HIPCHECK(hipMemcpyAsync(p->d.get(), p->image.data(), p->image.size(), hipMemcpyHostToDevice, h->stream.get()));
    *out = p.release();
    return SW_OK;
}

int sw_pssm_free(sw_pssm* p) {
    if (!p) return SW_OK;
    // scans in flight on the handle may still read the table
    (void)hipSetDevice(p->h->device);
    (void)quiesce(p->h);
    delete p;
    return SW_OK;
}

int sw_pssm_length(const sw_pssm* p, int32_t* qlen) {
    if (!p || !qlen) return fail(SW_E_INVALID, "null argument");
    *qlen = p->qlen;
    return SW_OK;
}

int sw_scan_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                 int32_t* scores_host) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return scan_host(h, db, pssm_src(p, gap_open, gap_extend), scores_host);
}

int sw_scan_pssm_topk(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                      int32_t k, int64_t* keys_host) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    const QuerySrc src = pssm_src(p, gap_open, gap_extend);
    return scan_topk_host(h, db, &src, 1, k, keys_host);
}

int sw_scan_pssm_topk_calib(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                            int32_t k, int64_t* keys_host, sw_calib* calib) {
    if (!calib) return fail(SW_E_INVALID, "null argument");
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    if (!db) return fail(SW_E_INVALID, "null argument");
    uint32_t* hist = nullptr;
    if (int rc = ensure_hist_host(h, 1, &hist)) return rc;
    const QuerySrc src = pssm_src(p, gap_open, gap_extend);
    if (int rc = scan_topk_host(h, db, &src, 1, k, keys_host, hist)) return rc;
    calib_of(db, hist, p->qlen, calib);
    return SW_OK;
}

int sw_scan_pssm_topk_ranked(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                             int32_t k, double max_evalue, int32_t* ids, int32_t* scores, sw_sig* sig, int32_t* nhits,
                             int64_t* n_pass, sw_calib* calib) {
    if (!scores) return fail(SW_E_INVALID, "null argument");
    int rc;
    if ((rc = check_pssm(h, p, gap_open, gap_extend))) return rc;
    if ((rc = check_ranked_args(h, db, 1, k, max_evalue, ids, sig, nhits, n_pass))) return rc;
    const QuerySrc src = pssm_src(p, gap_open, gap_extend);
    Ranked r;
    if ((rc = ranked_keys(h, db, &src, 1, k, max_evalue, 0, true, r))) return rc;
    const int32_t m = static_cast<int32_t>(std::min<int64_t>(k, r.count[0]));
    for (int32_t i = 0; i < m; ++i) {  // the gathered rows: {id, score, subject length, 0}
        ids[i] = r.rows[4 * i];
        scores[i] = r.rows[4 * i + 1];
        swcalib::significance(r.calib[0], r.rows[4 * i + 1], r.rows[4 * i + 2], &sig[i]);
    }
    *nhits = m;
    *n_pass = r.count[0];
    if (calib) *calib = r.calib[0];
    return SW_OK;
}

// ---- traceback --------------------------------------------------------------
int sw_align(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
             const int32_t* ids, int32_t n, sw_alignment* out, char* ops, int64_t ops_stride) {
    return align_impl(h, db, seq_src(query, qlen, sc), ids, n, out, ops, ops_stride, nullptr);
}

int sw_align_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                  const int32_t* ids, int32_t n, sw_alignment* out, char* ops, int64_t ops_stride) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return align_impl(h, db, pssm_src(p, gap_open, gap_extend), ids, n, out, ops, ops_stride, nullptr);
}

int sw_score_pair(sw_handle* h, const uint8_t* query, int32_t qlen, const uint8_t* subject, int32_t slen,
                  const sw_scoring* sc, int32_t* score) {
    if (!h || !score || slen < 0 || qlen < 0) return fail(SW_E_INVALID, "null argument");
    const int64_t offs[2] = {0, slen};
    const int32_t id = 0;
    sw_db* db = nullptr;
    int rc = sw_db_create(h, subject, offs, 1, &id, &db);
    if (rc) return rc;
    // a single pair takes the wavefront kernel (all subjects longer than 1)
    if ((rc = sw_db_set_long_threshold(db, 1))) { sw_db_free(db); return rc; }
    rc = sw_scan(h, db, query, qlen, sc, score);
    sw_db_free(db);
    return rc;
}

}  // extern "C"
