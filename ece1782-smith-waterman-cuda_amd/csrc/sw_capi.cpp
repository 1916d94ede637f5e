// sw_capi.cpp — the scan driver of the host driver (sw_driver.h): one scan's
// plan (sw_plan.cpp) enqueued stage by stage on the handle's streams, with
// the ranking and the calibration table that may ride on it, and the
// sw_scan*_device entry points.  The handle, the database, the scoring tables
// and everything layered on a scan are its sibling units (sw_handle.cpp,
// sw_db.cpp, sw_scoring.cpp, sw_search.cpp).
//
// The file keeps the name it had as the whole driver, for two reasons:
//   * bench.py hashes it (KERNEL_SOURCES) so that a stored traffic
//     measurement is reported only for the sources that decide the launches:
//     that is exactly the code in this file;
//   * it is the one object that carries the source id (sw_build_id below;
//     csrc/Makefile, tests/test_build.py).
//
// What the reference does per query (SWSolver.cu:266-404) and what replaces it:
//   * pad/encode the query and upload it to __constant__ (:267-299)
//       -> a 32 x qpad int8 query PROFILE (score of every residue code against
//          every query row, pre-biased by the gap for the linear kernels),
//          built on the device by the scan's first launch (sw_profile.hip)
//          from the query's codes (tiny: 32 B/row);
//   * re-pack the whole database into managed memory on every query,
//     longest-first, 32 lanes per block (:301-371)
//       -> packed once and kept resident (sw_db.cpp);
//   * launch in chunks with cudaDeviceSynchronize after each (:332-354,379)
//       -> one asynchronous launch per kernel on the handle's stream;
//   * read managed scores back in packing order (:383-390)
//       -> kernels write scores[id] directly.
#include <algorithm>
#include <cstdio>

#include "sw_calib.h"
#include "sw_driver.h"

using namespace swd;

namespace {

// fp16 represents every integer in [-kF16Span, kF16Span] exactly
constexpr int kF16Span = 2048;

// packed fp16 pair (v, v) of a small integer (|v| <= 2048: exact)
uint32_t f16_pair(int v) {
    const _Float16 x = static_cast<_Float16>(static_cast<float>(v));
    uint16_t b;
    std::memcpy(&b, &x, 2);
    return static_cast<uint32_t>(b) | (static_cast<uint32_t>(b) << 16);
}

// Record event k of the handle's current scan on stream s.
hipError_t mark(sw_handle* h, int k, hipStream_t s) {
    const hipError_t e = hipEventRecord(h->ev[k].get(), s);
    if (e == hipSuccess) *h->ev_rec |= 1u << k;
    return e;
}

// Read w0 (and w1, nullable) back on stream s as observation o, unless a
// readback is pending or o is the last one taken.
int readback_record(Readback& r, const Readback::Obs& o, const int32_t* w0, const int32_t* w1, hipStream_t s) {
    if (r.pending || (r.seen && r.last == o)) return SW_OK;
    if (!r.host.get()) {
        HostPtr<int32_t> host;
        Event ev;
        HIPCHECK(swk::host_alloc(host, 2 * sizeof(int32_t), hipHostMallocDefault));
        HIPCHECK(swk::event_create(ev, hipEventDisableTiming));
        r.host = std::move(host);
        r.ev = std::move(ev);
    }
    HIPCHECK(hipMemcpyAsync(r.host.get(), w0, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (w1) HIPCHECK(hipMemcpyAsync(r.host.get() + 1, w1, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipEventRecord(r.ev.get(), s));
    r.pending = true;
    r.sent = o;
    return SW_OK;
}

// True once per completed readback: r.host holds the words, r.last what they observe.
bool readback_take(Readback& r) {
    if (!r.pending || hipEventQuery(r.ev.get()) != hipSuccess) return false;
    r.pending = false;
    r.seen = true;
    r.last = r.sent;
    return true;
}

// ---- adaptive routing: what earlier scans of this database observed --------
// The intra chain's order.  Linear scoring with cheap gaps makes random
// pairs' scores grow with their lengths, so on long subjects the fp16 pass
// can flag many of them and its time on those is wasted.  Once a scan with
// the same scoring (skey) has flagged over a third of the long subjects at a
// query no longer than this one, the int16 form runs first, over all of them
// (the int16 cell costs ~1.4x the fp16 one, so fp16 first + int16 over the
// flagged fraction p wins while p < ~0.3).  The last observation is taken
// here once its readback has completed (long_pass records it).  opt =
// sw_opts intra_i16_first: 0 / 1 never / always, else the observations.
bool adapt_intra_i16_first(sw_db* db, uint64_t skey, int32_t qlen, int32_t opt) {
    if (readback_take(db->lcount) && 3 * static_cast<int64_t>(db->lcount.host.get()[0]) > db->shape.nlong) {
        const Readback::Obs& o = db->lcount.last;
        bool seen = false;
        for (auto& e : db->i16_first)
            if (e.first == o.key) {
                e.second = std::min(e.second, o.qlen);
                seen = true;
            }
        if (!seen) db->i16_first.emplace_back(o.key, o.qlen);
    }
    if (opt == 0 || opt == 1) return opt == 1;
    for (const auto& e : db->i16_first)
        if (e.first == skey && e.second <= qlen) return true;
    return false;
}

// The same for the inter scan, per block: long queries under cheap linear
// gaps put the WIDEST blocks (length-sorted, ids 0, 1, ...) in the fp16
// guard band, and their re-scoring by the list kernel (one wave per block,
// every pass in turn) takes longer than the whole scan.  A scan with the
// same scoring whose fp16 pass flagged most of blocks [0, span) makes
// later queries at least as long run those blocks in int16, by wave pairs
// beside the fp16 launch.  opt = sw_opts inter_i16_span: n forces n blocks (0: off).
int32_t adapt_inter_i16_span(sw_db* db, uint64_t skey, int32_t qlen, int32_t opt) {
    if (readback_take(db->icount)) {
        const Readback::Obs& o = db->icount.last;
        const int32_t cnt = db->icount.host.get()[0], span = db->icount.host.get()[1] + 1;
        // most of [nr, span) flagged: not a few high-scoring hits far out
        if (cnt > 0 && span > o.nr && 2 * static_cast<int64_t>(cnt) >= span - o.nr) {
            // keep a staircase per scoring: drop what the new observation
            // dominates (a query at least as long with a span no larger),
            // skip it if an existing one dominates it
            bool dominated = false;
            for (const auto& e : db->i16_span)
                if (e.key == o.key && e.qlen <= o.qlen && e.span >= span) dominated = true;
            if (!dominated) {
                db->i16_span.erase(std::remove_if(db->i16_span.begin(), db->i16_span.end(),
                                                  [&](const sw_db::SpanObs& e) {
                                                      return e.key == o.key && e.qlen >= o.qlen && e.span <= span;
                                                  }),
                                   db->i16_span.end());
                db->i16_span.push_back({o.key, o.qlen, span});
            }
        }
    }
    int32_t i16_span = 0;
    if (opt >= 0) {
        i16_span = opt;
    } else {
        for (const auto& o : db->i16_span)
            if (o.key == skey && o.qlen <= qlen) i16_span = std::max(i16_span, o.span);
    }
    return static_cast<int32_t>(std::min<int64_t>(std::max(i16_span, 0), db->shape.nblocks));
}

// Query profiles.  Inter kernel: prof[c][i] = S[q_i][c] (+ gap for the
// linear kernels) for residue codes c < 25; rows c >= 25 (the pad code) and
// columns i >= qlen score 0 (+ gap).  A zero-score pad row/column can never
// raise the maximum (every such cell is <= max(0, its diagonal, its gap
// predecessors)).  Intra kernel: the same values laid out per chunk of
// 64*ri query rows as [code][lane][RIP] so each lane's ri rows are contiguous.
struct Profiles {
    int8_t* dev = nullptr;  // device copy of this scan's profiles
    int32_t stride = 0;      // inter profiles: entries per code row
    size_t off8 = 0;         // int8 inter profile (biased for linear)
    size_t off16 = 0;        // int16 inter profile (packed kernels)
    size_t intra_off = 0;    // lane-slotted intra profile
    size_t total = 0;
    int slot = 0;            // the handle's profile slot holding them
};

// Built on the device (swk::sw_build_profile, one launch per 2,048 query
// rows; the first also zeroes the rescue lists' counters `reset`) in one of
// the handle's profile slots, on the scan's stream.
// A PSSM's profiles come from its resident table (sw_build_profile_pssm): one
// launch whatever the query length, nothing copied from the host.
int build_profiles(sw_handle* h, const QuerySrc& src, const int8_t* mat, int go, bool affine,
                   int32_t qpad_inter, bool want16, int ri, int32_t qpad_intra, int32_t* const (&reset)[10],
                   Profiles* P) {
    const uint8_t* q = src.codes;
    const int32_t qlen = src.qlen;
    for (int32_t i = 0; i < qlen && !src.pssm; ++i)
        if (q[i] >= SW_ALPHABET) return fail(SW_E_INVALID, "query residue code out of range (use sw_encode)");
    P->stride = static_cast<int32_t>(round_up(std::max<int32_t>(qpad_inter, 16), 16));
    const size_t n = static_cast<size_t>(swk::kProfileRows) * P->stride;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at = round_up(static_cast<int64_t>(at + bytes), 256);
        return o;
    };
    P->off8 = take(n);
    P->off16 = want16 ? take(2 * n) : 0;
    const size_t intra_bytes = ri ? static_cast<size_t>(qpad_intra / (swk::kLanes * ri)) * swk::intra_chunk_bytes(ri) : 0;
    P->intra_off = take(intra_bytes);
    P->total = at;
    P->slot = h->prof_next;
    sw_handle::ProfSlot& S = h->prof[h->prof_next];
    h->prof_next = (h->prof_next + 1) % sw_handle::kProfSlots;
    if (S.pending) HIPCHECK(hipEventSynchronize(S.last_end));
    S.pending = false;
    if (P->total > S.dcap) {
        if (S.d.get()) {
            HIPCHECK(hipStreamSynchronize(h->stream.get()));  // scans in flight may still read it
            if (S.tail_pending) HIPCHECK(hipEventSynchronize(S.tail_read.get()));
            S.tail_pending = false;
            S.d.reset();
        }
        S.dcap = std::max<size_t>(P->total, 1 << 16);
        HIPCHECK(swk::dev_alloc(S.d, S.dcap));
    }
    P->dev = S.d.get();
    // on the scan's stream: after the scans before it (the slot's last
    // reader among them), before this one
    if (S.tail_pending) {  // a deferred tail still reads the slot's last profiles
        HIPCHECK(hipStreamWaitEvent(h->stream.get(), S.tail_read.get(), 0));
        S.tail_pending = false;
    }
    // what the two launch forms' arguments share
    auto images = [&](auto& a) {
        a.p8 = S.d.get() + P->off8;
        a.p16 = want16 ? reinterpret_cast<int16_t*>(S.d.get() + P->off16) : nullptr;
        a.pin = ri ? S.d.get() + P->intra_off : nullptr;
        a.stride = P->stride;
        a.qlen = qlen;
        a.bias = affine ? 0 : go;
        a.ri = ri;
        a.rip = swk::intra_rip(ri);
        a.qpad_intra = ri ? qpad_intra : 0;
        for (int k = 0; k < 10; ++k) a.reset[k] = reset[k];
        return std::max(P->stride, a.qpad_intra);  // the rows to build
    };
    if (src.pssm) {
        swk::PssmProfileArgs a{};
        a.rows = images(a);
        a.pssm = src.pssm->d.get();
        a.ld = src.pssm->ld;
        HIPCHECK(swk::launch_build_profile_pssm(a, h->stream.get()));
    } else {
        swk::ProfileArgs a{};
        const int32_t rows = images(a);
        std::memcpy(a.mat, mat, 625);
        for (int32_t r0 = 0; r0 < rows; r0 += swk::kProfQueryChunk) {
            a.row0 = r0;
            a.row1 = std::min(rows, r0 + swk::kProfQueryChunk);
            const int32_t nq = std::max(0, std::min(a.row1, qlen) - r0);
            if (nq) std::memcpy(a.q, q + r0, static_cast<size_t>(nq));
            HIPCHECK(swk::launch_build_profile(a, h->stream.get()));
            for (auto& p : a.reset) p = nullptr;  // once
        }
    }
    S.last_end = h->ev[3].get();  // recorded at the end of this scan (scan_impl)
    S.pending = true;
    h->open_slot = P->slot;  // until ev[3] is recorded (scan_impl cleans up if it fails first)
    return SW_OK;
}

// The work table of sw_scan_lpt for this scan's shape (built once, cached,
// the oldest of 8 dropped); null after an error.
const sw_db::LptTable* lpt_table(sw_db* db, const swplan::ScanPlan& p) {
    const sw_opts& O = db->h->opts;
    const bool tri = p.ntri != 0;
    for (const auto& t : db->lay.lpt_tables)
        if (t.qpad == p.qpad_inter && t.rows == p.lpt_rows && t.qpad_intra == p.qpad_intra2 && t.ri == p.ri2 &&
            t.npair == p.npair && t.group == p.nquad && t.tail == p.ntail && t.pipe_opt == O.lpt_pipe &&
            t.affine == p.affine && t.tri == tri && t.tail_opt == O.lpt_pipe_tail)
            return &t;
    const swplan::LptPlan pl = swplan::lpt_plan(plan_view(db), p.qpad_inter, p.lpt_rows, p.qpad_intra2, p.ri2, p.npair,
                                                p.nquad, p.ntail, p.affine, tri);
    sw_db::LptTable t{p.qpad_inter, p.lpt_rows, p.qpad_intra2, p.ri2, p.npair, p.nquad, p.ntail,
                      static_cast<int32_t>(pl.order.size()), p.affine, tri, pl.npipe, O.lpt_pipe, pl.pipe_tail,
                      O.lpt_pipe_tail, DevPtr<int32_t>{}, pl.cost};
    const size_t bytes = pl.order.size() * sizeof(int32_t);
    hipError_t e = swk::dev_alloc(t.d_order, bytes);
    if (e == hipSuccess) e = hipMemcpy(t.d_order.get(), pl.order.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fail(SW_E_HIP, std::string("sw_scan_lpt's work table: ") + hipGetErrorString(e));
        return nullptr;
    }
    db->lay.device_bytes += bytes;
    if (db->lay.lpt_tables.size() >= 8) db->lay.lpt_tables.erase(db->lay.lpt_tables.begin());
    db->lay.lpt_tables.push_back(std::move(t));
    return &db->lay.lpt_tables.back();
}

// The device copy of a merged launch's drain arguments (swk::DrainArgs: read
// from the kernel arguments, the drain's values stayed in registers across
// the scan loops and spilled).  `key` lists everything the content is a
// function of (profile slot, list parity, score buffer, query length,
// scoring, split); a miss uploads the content in stream order, a hit (every
// scan of a steady loop after the first few) costs no copy.
int drain_blob(sw_db* db, hipStream_t s, const std::vector<uint64_t>& key, const swk::DrainArgs& d,
               const swk::DrainArgs** out) {
    if (!db->lay.d_drain.get()) {  // both or neither
        DevPtr<swk::DrainArgs> dev;
        HIPCHECK(swk::dev_alloc(dev, sw_db::kDrainSlots * sizeof(swk::DrainArgs)));
        HIPCHECK(swk::host_alloc(db->lay.h_drain, sw_db::kDrainSlots * sizeof(swk::DrainArgs), hipHostMallocDefault));
        db->lay.d_drain = std::move(dev);
        db->lay.device_bytes += sw_db::kDrainSlots * sizeof(swk::DrainArgs);
    }
    for (size_t k = 0; k < db->lay.drain_keys.size(); ++k)
        if (db->lay.drain_keys[k] == key) {
            *out = db->lay.d_drain.get() + k;
            return SW_OK;
        }
    // a slot is rewritten only after the 31 uploads since its last one, each
    // in stream order behind the scans that read it
    const int k = db->lay.drain_next;
    db->lay.drain_next = (k + 1) % sw_db::kDrainSlots;
    if (static_cast<int>(db->lay.drain_keys.size()) <= k) db->lay.drain_keys.resize(k + 1);
    db->lay.drain_keys[k] = key;
    db->lay.h_drain.get()[k] = d;
    HIPCHECK(hipMemcpyAsync(db->lay.d_drain.get() + k, &db->lay.h_drain.get()[k], sizeof d, hipMemcpyHostToDevice, s));
    *out = db->lay.d_drain.get() + k;
    return SW_OK;
}

// A scan's ranking: a top-K launch on the scan's stream after every stage
// that writes its scores, over the database's subjects: its scores through
// the result ids, or directly when those are the identity.
int rank_after(sw_handle* h, sw_db* db, const int32_t* scores_dev, const RankReq& rq) {
    swk::TopkSrc src{};
    src.scores = scores_dev;
    src.gid = rq.gid;
    src.id_base = rq.id_base;
    int rc;
    if ((rc = subject_ids(db, &src.rid))) return rc;
    if ((rc = ensure_topk_work(h, swk::topk_workspace_bytes(db->n, rq.k)))) return rc;
    HIPCHECK(swk::launch_topk(src, db->n, rq.k, rq.out, h->d_topk_work.get(), h->stream.get()));
    ++h->launches;
    return SW_OK;
}

// ---- one scan: the plan (swplan::scan_plan), then its enqueue stages -------
// Boundary rows: inter H, F; intra H, F.
struct BndRows {
    int32_t *h, *f, *lh, *lf;
};
// ... of a scan's passes, and of the rescue tails in stream order behind them
BndRows pass_rows(const sw_db::Layout& l) { return {l.d_bnd_h.get(), l.d_bnd_f.get(), l.d_lbnd_h.get(), l.d_lbnd_f.get()}; }
// ... of a deferred rescue tail, and of the merged launch's drain (ensure_rbnd)
BndRows tail_rows(const sw_db::Layout& l) { return {l.d_rbnd_h.get(), l.d_rbnd_f.get(), l.d_rlbnd_h.get(), l.d_rlbnd_f.get()}; }

// What the stages of one scan share.
struct Scan {
    sw_handle* h = nullptr;
    sw_db* db = nullptr;
    swplan::ScanPlan plan;
    swplan::PlanScoring sc;
    int32_t qlen = 0;
    uint64_t skey = 0, qhash = 0;  // FNV-1a of the scoring and of the query (what the readbacks observe)
    int32_t* scores = nullptr;
    // this scan's list set (scan_lists): inter lists A and B [count, ids...],
    // the largest flagged block, the drain's dequeue heads of A and B; intra
    // lists 1 (flagged by the fp16 pass) and 2 (... and again by int16), their
    // heads; the merged launch's work counter (persistent form)
    int par = 0;
    int32_t *listA = nullptr, *listB = nullptr, *maxA = nullptr, *headA = nullptr;
    int32_t *list1 = nullptr, *list2 = nullptr, *head1 = nullptr;
    int32_t* lpt_next = nullptr;
    bool deferred = false;  // the rescue tail runs on its own stream and boundary rows (sw_handle::tail)
    Profiles P;
    // the arguments of the main inter launch, of the int32 long-subject
    // kernel and of the fp16 / int16 one (scan_args); every other launch of
    // the scan derives its own from these
    swk::InterArgs a{};
    swk::IntraArgs ia{}, x{};
    bool inter_tail = false, intra_tail = false;  // rescue stages are left to launch after the passes
};

// Empty query: every score is 0 (the reference's kernel leaves maxScore 0).
int scan_empty(sw_handle* h, sw_db* db, int32_t* scores_dev, bool defer, const RankReq* rq, uint32_t* hist) {
    int rc;
    db->last_ncoop = 0;
    db->last_npair = 0;
    h->last_kernel = "none";
    h->last_intra = "none";
    // a non-deferred scan completes on the handle's stream: so do the
    // earlier scans' deferred tails (a batch may end with an empty query)
    if (!defer && (rc = join_tails(h))) return rc;
    HIPCHECK(mark(h, 0, h->stream.get()));
    if (db->max_id >= 0) HIPCHECK(hipMemsetAsync(scores_dev, 0, static_cast<size_t>(db->max_id + 1) * 4, h->stream.get()));
    if (rq && (rc = rank_after(h, db, scores_dev, *rq))) return rc;
    if (hist && (rc = hist_after(h, db, scores_dev, hist))) return rc;
    for (int k = 1; k < 8; ++k) HIPCHECK(mark(h, k, h->stream.get()));
    h->timed = true;
    return SW_OK;
}

// The rescue lists of this scan (allocated on first need, re-initialised
// after a fault), the boundary rows, and where the rescue tail runs.
int scan_lists(Scan& c, bool defer) {
    sw_handle* h = c.h;
    sw_db* db = c.db;
    const swplan::ScanPlan& p = c.plan;
    int rc;
    // lists A and B, the largest flagged block, a spare word, the dequeue
    // heads of A and B (the merged launch's drain); every entry starts at -1
    // (sw_kernels.h: whoever takes an entry resets it)
    const int64_t rstride = 2 * (db->shape.nblocks + 1) + 4;
    const int64_t lstride = 2 * (db->shape.nlong + 1) + 2;  // intra lists 1 and 2, their heads
    if (p.rescue && db->shape.nblocks && !db->lay.d_rescue.get()) {
        HIPCHECK(swk::dev_alloc(db->lay.d_rescue, 2 * rstride * sizeof(int32_t)));
        HIPCHECK(hipMemsetAsync(db->lay.d_rescue.get(), 0xff, 2 * rstride * sizeof(int32_t), h->stream.get()));
        db->lay.device_bytes += 2 * rstride * sizeof(int32_t);
    }
    if ((p.multi_inter || p.multi_intra) && (rc = ensure_bnd(db, p.affine, p.intra_x2))) return rc;
    if (p.intra_x2 && !db->lay.d_lrescue.get()) {  // two lists: [count, subjects...] x 2
        HIPCHECK(swk::dev_alloc(db->lay.d_lrescue, 2 * lstride * sizeof(int32_t)));
        HIPCHECK(hipMemsetAsync(db->lay.d_lrescue.get(), 0xff, 2 * lstride * sizeof(int32_t), h->stream.get()));
        db->lay.device_bytes += 2 * lstride * sizeof(int32_t);
    }
    if (db->list_epoch != fault_epoch()) {  // a fault since: entries may be left claimed
        if ((rc = join_tails(h))) return rc;
        hipStream_t const s = h->stream.get();
        if (int32_t* l = db->lay.d_rescue.get()) HIPCHECK(hipMemsetAsync(l, 0xff, 2 * rstride * sizeof(int32_t), s));
        if (int32_t* l = db->lay.d_lrescue.get()) HIPCHECK(hipMemsetAsync(l, 0xff, 2 * lstride * sizeof(int32_t), s));
        db->list_epoch = fault_epoch();
    }
    // this scan's list set; a deferred tail of the scan before last used it
    c.par = h->parity;
    h->parity ^= 1;
    if (h->tail_pending[c.par]) {
        HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->tail_done[c.par].get(), 0));
        h->tail_pending[c.par] = false;
    }
    // The drain re-scores on the deferred tails' boundary rows (d_rbnd_*,
    // d_rlbnd_*): a non-merged scan just before this one (a longer query
    // routed int16-first, say) may still be running its tail on those rows,
    // so the merged launch starts after every pending tail.
    if (p.drain && (rc = join_tails(h))) return rc;
    if (db->lay.d_rescue.get()) {
        c.listA = db->lay.d_rescue.get() + c.par * rstride;
        c.listB = c.listA + db->shape.nblocks + 1;
        c.maxA = c.listA + 2 * (db->shape.nblocks + 1);
        c.headA = c.maxA + 2;
        if (p.lpt && h->opts.lpt_persist != 0) c.lpt_next = c.maxA + 1;  // the spare word
    }
    if (db->lay.d_lrescue.get()) {
        c.list1 = db->lay.d_lrescue.get() + c.par * lstride;
        c.list2 = c.list1 + db->shape.nlong + 1;
        c.head1 = c.list2 + db->shape.nlong + 1;
    }
    c.deferred = !p.drain && defer && (!(p.multi_inter || p.multi_intra) || ensure_rbnd(db, p.affine, p.intra_x2));
    return SW_OK;
}

// The profiles, and the rescue lists' counters (inter A, B, largest flagged
// block; intra 1, 2; the drain's heads; the work counter) zeroed by the same
// launch, before the fork so the side streams see them.
int scan_profiles(Scan& c, const QuerySrc& src, const int8_t* mat) {
    const swplan::ScanPlan& p = c.plan;
    const bool d = p.drain;
    int32_t* const cA = (p.rescue && c.db->shape.nblocks) ? c.listA : nullptr;
    int32_t* const c1 = p.intra_x2 ? c.list1 : nullptr;
    int32_t* const reset[10] = {cA, (cA && p.f16) ? c.listB : nullptr, (cA && p.f16) ? c.maxA : nullptr, c1,
                                c1 ? c.list2 : nullptr, d ? c.headA : nullptr, d ? c.headA + 1 : nullptr,
                                d ? c.head1 : nullptr, d ? c.head1 + 1 : nullptr, c.lpt_next};
    const int rc = build_profiles(c.h, src, mat, c.sc.go, p.affine,
                                  std::max({p.qpad_inter, p.qpad_rescue, p.qpad_coop, p.qpad_list, p.qpad_intra2}),
                                  p.shape.x2s || p.intra_x2, p.ri, p.qpad_intra, reset, &c.P);
    c.h->evpool[c.h->nscans - 1].merged = p.lpt;
    return rc;
}

// c.a: the main inter launch (per-wave; wave groups + single waves; merged).
int inter_args(Scan& c) {
    sw_db* db = c.db;
    const swplan::ScanPlan& p = c.plan;
    const int go = c.sc.go, ge = c.sc.ge;
    swk::InterArgs& a = c.a;
    a.residues = db->lay.d_res.get();
    a.blk_off = db->lay.d_blk_off.get();
    a.blk_groups = db->lay.d_blk_groups.get();
    a.blk_cols = db->lay.d_blk_cols.get();
    a.lane_ids = db->lay.d_lane_ids.get();
    a.nblocks = static_cast<int32_t>(db->shape.nblocks);
    a.prof = c.P.dev + (p.shape.x2s ? c.P.off16 : c.P.off8);
    a.prof_stride = c.P.stride;
    a.qpad = p.qpad_inter;
    a.gap_open = go;
    a.gap_extend = ge;
    a.bnd_h = db->lay.d_bnd_h.get();
    a.bnd_f = db->lay.d_bnd_f.get();
    a.scores = c.scores;
    if (c.h->opts.trace_file[0]) {
        if (!db->lay.h_trace.get()) {
            // one entry per block, then one per workgroup of a merged
            // launch (at most nblocks inter + nlong / 8 intra workgroups)
            db->lay.trace_entries = static_cast<size_t>(2 * db->shape.nblocks + db->shape.nlong + 8);
            HIPCHECK(swk::host_alloc(db->lay.h_trace, 32 * db->lay.trace_entries, hipHostMallocMapped));
            std::memset(db->lay.h_trace.get(), 0, 32 * db->lay.trace_entries);
        }
        HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&a.trace), db->lay.h_trace.get(), 0));
    }
    if (p.rescue) {
        a.rescue_count = c.listA;
        a.rescue_list = c.listA + 1;
        if (p.f16) a.rescue_max = c.maxA;  // counters reset before the fork
        // The biased cell stores true + bias + Z as unsigned integers that
        // are positive normal fp16 patterns (swplan::cell_range states the
        // bounds; matrix and table entries are int8, validated to -100..100,
        // so -128 bounds them).
        const swplan::CellRange cr = swplan::cell_range(-128, c.sc.max_s, go, ge);
        a.sat_limit = cr.sat_limit;
        std::copy(std::begin(cr.step), std::end(cr.step), a.f16_step);
        a.f16_gog = cr.gog;
        a.f16_zero = cr.step[0];
        std::copy(std::begin(cr.diff), std::end(cr.diff), a.f16_diff);
    }
    a.re_last = p.re_last;  // the short last pass (x2s_pass)
    // its blocks: [blk_base, blk_first) by wave groups (the merged launch:
    // quads or tris first, the narrowest by tail pairs), one wave per block
    // from blk_first on; blocks below run beside it (coop, int16 pairs)
    if (p.lpt) {
        a.blk_first = p.npair;
        a.blk_quad = p.nquad;
        a.blk_tri = p.ntri ? 1 : 0;
        a.blk_tail = static_cast<int32_t>(db->shape.nblocks) - p.ntail;
    } else if (p.npair) {
        a.blk_base = p.nr;
        a.blk_first = std::max(p.npair, p.nr);
    } else {
        a.blk_first = p.ncoop;
    }
    return SW_OK;
}

// c.ia: the int32 kernel over the long subjects.
void intra_args(Scan& c) {
    const sw_db* db = c.db;
    swk::IntraArgs& ia = c.ia;
    ia.residues = db->lay.d_lres.get();
    ia.subj_off = db->lay.d_loff.get();
    ia.subj_len = db->lay.d_llen.get();
    ia.subj_id = db->lay.d_lid.get();
    ia.nsubj = static_cast<int32_t>(db->shape.nlong);
    ia.prof = c.P.dev + c.P.intra_off;
    ia.qpad = c.plan.qpad_intra;
    ia.gap_open = c.sc.go;
    ia.gap_extend = c.sc.ge;
    ia.bnd_h = db->lay.d_lbnd_h.get();
    ia.bnd_f = db->lay.d_lbnd_f.get();
    ia.scores = c.scores;
}

// c.x: the two-subjects kernel's first pass, fp16 flagging into list 1 (or
// int16 over every subject, flagging into list 2).
void intra_x2_args(Scan& c) {
    const swplan::ScanPlan& p = c.plan;
    const int go = c.sc.go, ge = c.sc.ge;
    swk::IntraArgs& x = c.x;
    x = c.ia;
    x.prof = c.P.dev + c.P.off16;
    x.prof_stride = c.P.stride;
    x.bias = p.affine ? 0 : go;  // the linear profile holds S + gap
    x.qpad = p.qpad_intra2;
    // biased cell: stored values up to (RI + 10) ge above the true ones,
    // offset by zero = -2048 + 2 ge as the inter cell's (the lowest value
    // an addition reads is a rebased row -1 H of bias -2 ge: exact)
    const int zero = -kF16Span + 2 * ge;
    x.sat_limit = kF16Span - zero - 2 * std::max(c.sc.max_s, 1) - swk::intra_bias_rows(p.ri2) * ge;
    for (int j = 0; j < swk::kIntraSteps; ++j) x.f16_step[j] = f16_pair(j * ge + zero);
    x.f16_zero = f16_pair(zero);
    x.f16_gog = f16_pair(go - ge);
    int32_t* const flagged = p.intra_i16_first ? c.list2 : c.list1;
    x.rescue_count = flagged;
    x.rescue_list = flagged + 1;
}

int scan_args(Scan& c) {
    if (c.db->shape.nlong) {
        intra_args(c);
        if (c.plan.intra_x2) intra_x2_args(c);
    }
    return c.db->shape.nblocks ? inter_args(c) : SW_OK;
}

// The four rescue stages, on boundary rows r:
//   a16  int16 blocks over list A, flagging near-32767 ones into list B (fp16 scans);
//   a32  int32 blocks over list B (list A for the int16 scans);
//   i16  int16 subject pairs over list 1, flagging into list 2;
//   i32  int32 subjects over list 2.
// x: the fp16 pass's arguments as launched.  Launched as the scan's rescue
// tail (launch_inter_tail, launch_intra_tail), or in_launch: run by the
// merged launch itself (swk::DrainArgs), which takes its entries from
// DrainArgs::lists instead of the stages' list fields and keeps the block
// timeline (trace) and the largest flagged block to its fp16 pass.
struct RescueStages {
    swk::InterArgs a16, a32;
    swk::IntraArgs i16, i32;
};
RescueStages rescue_stages(const Scan& c, const swk::IntraArgs& x, const BndRows& r, bool in_launch) {
    const swplan::ScanPlan& p = c.plan;
    auto items = [](int32_t* list) { return list ? list + 1 : nullptr; };
    int32_t* const l32 = p.f16 ? c.listB : c.listA;
    RescueStages s{c.a, c.a, x, c.ia};
    s.a16.bnd_h = s.a32.bnd_h = r.h;
    s.a16.bnd_f = s.a32.bnd_f = r.f;
    s.a16.qpad = p.qpad_list;
    // (the rescue stages keep full-height passes: the list kernel pads the
    // query to its own pass height)
    s.a16.re_last = p.affine ? 32 : 48;
    s.a32.re_last = swplan::rescue_rows(p.affine);  // (the int32 kernels have one form)
    s.a16.rescue_list = items(c.listB);
    s.a16.rescue_count = c.listB;
    s.a16.rescue_max = nullptr;
    s.a32.prof = c.P.dev + c.P.off8;
    s.a32.qpad = p.qpad_rescue;
    s.a32.rescue_list = nullptr;
    s.a32.rescue_count = nullptr;
    s.i16.bnd_h = s.i32.bnd_h = r.lh;
    s.i16.bnd_f = s.i32.bnd_f = r.lf;
    s.i16.rescue_list = items(c.list2);
    s.i16.rescue_count = c.list2;
    if (in_launch) {
        s.a16.trace = s.a32.trace = nullptr;
        s.a32.rescue_max = nullptr;
    } else {
        s.a16.blk_list = items(c.listA);
        s.a16.blk_count = c.listA;
        s.a32.blk_list = items(l32);
        s.a32.blk_count = l32;
        s.i16.subj_list = items(c.list1);
        s.i16.list_count = c.list1;
        s.i32.subj_list = items(c.list2);
        s.i32.list_count = c.list2;
    }
    return s;
}

// The inter scan's rescue tail on stream st: the int16 packed kernel over
// the blocks the fp16 kernel flagged (scores near 2048), then int32 over
// what that flags (near 32767).
int launch_inter_tail(Scan& c, hipStream_t st, const RescueStages& s) {
    if (c.plan.f16) {
        HIPCHECK(swk::launch_inter_x2s_list(s.a16, c.plan.affine, st));
        ++c.h->launches;
    }
    HIPCHECK(swk::launch_inter_rescue(s.a32, c.plan.affine, st));
    ++c.h->launches;
    return SW_OK;
}

// The long subjects' rescue tail on stream st: the int16 form over the fp16
// pass's list (high-scoring pairs, or linear scoring with cheap gaps), then
// int32 over what is left (device-side list).
int launch_intra_tail(Scan& c, hipStream_t st, const RescueStages& s) {
    if (!c.plan.intra_i16_first) {
        HIPCHECK(swk::launch_intra_x2_list16(s.i16, c.plan.ri2, st));
        ++c.h->launches;
    }
    HIPCHECK(swk::launch_intra(s.i32, c.plan.ri, c.plan.affine, st));
    ++c.h->launches;
    return SW_OK;
}

// After the long subjects' first pass on stream is: its rescue stages right
// behind it, or deferred to the tail stream (deferred_tails).
int intra_tail(Scan& c, hipStream_t is) {
    c.intra_tail = true;
    if (c.deferred) {
        HIPCHECK(hipEventRecord(c.h->side_done.get(), is));
        return SW_OK;
    }
    return launch_intra_tail(c, is, rescue_stages(c, c.x, pass_rows(c.db->lay), false));
}

// After every fp16 launch that appends to list A has joined the main
// stream: the flagged count and largest flagged block, read by a later scan
// (adapt_inter_i16_span), and the inter rescue stages as intra_tail's.
int inter_tail(Scan& c) {
    sw_handle* h = c.h;
    const swplan::ScanPlan& p = c.plan;
    int rc;
    if (p.f16 && p.rescue &&
        (rc = readback_record(c.db->icount, {c.skey, c.qhash, c.qlen, p.nr}, c.listA, c.maxA, h->stream.get())))
        return rc;
    c.inter_tail = p.rescue && !p.drain;
    if (!c.inter_tail) return SW_OK;
    if (c.deferred) {
        HIPCHECK(hipEventRecord(h->main_done.get(), h->stream.get()));
        return SW_OK;
    }
    return launch_inter_tail(c, h->stream.get(), rescue_stages(c, c.x, pass_rows(c.db->lay), false));
}

// The long subjects on the side stream, beside the inter kernels.
int long_pass(Scan& c) {
    sw_handle* h = c.h;
    const swplan::ScanPlan& p = c.plan;
    hipStream_t const is = h->side.get();
    int rc;
    HIPCHECK(hipStreamWaitEvent(is, h->ev[0].get(), 0));
    h->had_intra = true;
    ++h->launches;
    if (!p.intra_x2) {  // int32 over every long subject
        HIPCHECK(swk::launch_intra(c.ia, p.ri, p.affine, is));
        return SW_OK;
    }
    if (p.intra_i16_first) {
        // the int16 form over every long subject, flagging near-32767 ones
        HIPCHECK(swk::launch_intra_x2_int16(c.x, p.ri2, is));
    } else {
        HIPCHECK(swk::launch_intra_x2(c.x, p.ri2, is));
        // the fp16 pass's flagged count, read by a later scan (adapt_intra_i16_first)
        if ((rc = readback_record(c.db->lcount, {c.skey, c.qhash, c.qlen, 0}, c.list1, nullptr, is))) return rc;
    }
    return intra_tail(c, is);
}

// The inter blocks on the main stream: the widest by the cooperative kernel
// or (the adaptive span) in int16 by wave pairs on a stream of their own,
// the rest in one launch.
int inter_pass(Scan& c) {
    sw_handle* h = c.h;
    const swplan::ScanPlan& p = c.plan;
    if (p.ncoop) {
        // on its own stream, so the per-wave kernel fills the GPU beside it
        swk::InterArgs k = c.a;
        k.blk_first = 0;
        k.qpad = p.qpad_coop;
        k.prof = c.P.dev + c.P.off8;  // the coop kernel reads the int8 profile
        HIPCHECK(hipStreamWaitEvent(h->side2.get(), h->ev[0].get(), 0));
        HIPCHECK(mark(h, 4, h->side2.get()));
        HIPCHECK(swk::launch_inter_coop(k, p.ncoop, p.affine, h->opts.coop_skew != 0, h->side2.get()));
        HIPCHECK(mark(h, 5, h->side2.get()));
        HIPCHECK(hipEventRecord(h->coop_done.get(), h->side2.get()));
        ++h->launches;
    } else if (p.nr) {
        // blocks [0, nr) in int16 by wave pairs beside the fp16 launch;
        // their near-32767 ones go to list B (the int32 stage)
        swk::InterArgs k = c.a;
        k.nblocks = p.nr;
        k.blk_base = 0;
        k.blk_first = 0;
        k.rescue_list = c.listB + 1;
        k.rescue_count = c.listB;
        k.rescue_max = nullptr;
        HIPCHECK(hipEventRecord(h->fork2.get(), h->stream.get()));
        HIPCHECK(hipStreamWaitEvent(h->side2.get(), h->fork2.get(), 0));
        HIPCHECK(mark(h, 4, h->side2.get()));
        HIPCHECK(swk::launch_inter_x2p(k, p.affine, false, false, 2, h->side2.get()));
        HIPCHECK(mark(h, 5, h->side2.get()));
        HIPCHECK(hipEventRecord(h->coop_done.get(), h->side2.get()));
        ++h->launches;
    }
    HIPCHECK(mark(h, 6, h->stream.get()));
    if (p.npair)  // one launch: pairs for blocks [nr, npair), one wave per block after
        HIPCHECK(swk::launch_inter_x2p(c.a, p.affine, p.f16, true, swplan::pair_group(plan_view(c.db)), h->stream.get()));
    else
        HIPCHECK(swk::launch_inter(c.a, p.affine, p.shape, h->stream.get()));
    HIPCHECK(mark(h, 7, h->stream.get()));
    ++h->launches;
    if (p.ncoop || p.nr) HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->coop_done.get(), 0));
    return inter_tail(c);
}

// The merged launch's drain arguments (swk::DrainArgs): the four rescue
// stages on the tails' boundary rows, as a device blob (drain_blob).
int drain_args(Scan& c, const swk::IntraArgs& x, const sw_db::LptTable& t, const swk::DrainArgs** out) {
    const swplan::ScanPlan& p = c.plan;
    const RescueStages s = rescue_stages(c, x, tail_rows(c.db->lay), true);
    swk::DrainArgs d{};
    d.a16 = s.a16;
    d.a32 = s.a32;
    d.i16 = s.i16;
    d.i32 = s.i32;
    d.lists[0] = c.listA;
    d.lists[1] = c.listB;
    d.lists[2] = c.list1;
    d.lists[3] = c.list2;
    d.heads[0] = c.headA;
    d.heads[1] = c.headA + 1;
    d.heads[2] = c.head1;
    d.heads[3] = c.head1 + 1;
    d.fault = c.h->d_fault;
    d.spin = c.h->opts.drain_spin >= 0 ? c.h->opts.drain_spin : (1 << 22);
    // (every field of d the blob's bytes depend on)
    const std::vector<uint64_t> key = {
        reinterpret_cast<uint64_t>(c.P.dev), c.P.off8, c.P.off16, c.P.intra_off, static_cast<uint64_t>(c.par),
        reinterpret_cast<uint64_t>(c.scores), static_cast<uint64_t>(c.qlen), c.skey,
        static_cast<uint64_t>(p.npair) | static_cast<uint64_t>(c.a.blk_tri) << 32,
        static_cast<uint64_t>(p.nquad) | static_cast<uint64_t>(p.ntail) << 32,
        static_cast<uint64_t>(c.P.stride),
        reinterpret_cast<uint64_t>(c.a.trace),
        static_cast<uint64_t>(p.ri2) | static_cast<uint64_t>(p.lpt_rows) << 16 | static_cast<uint64_t>(t.npipe) << 32,
        static_cast<uint64_t>(static_cast<uint32_t>(t.pipe_tail)),
        static_cast<uint64_t>(static_cast<uint32_t>(d.spin))};
    return drain_blob(c.db, c.h->stream.get(), key, d, out);
}

// One launch on the main stream: the inter groups + single waves and the
// long subjects' fp16 pass, longest work first (sw_scan_lpt); draining, it
// runs the rescue stages too, else they follow in stream order or deferred.
int merged_pass(Scan& c) {
    sw_handle* h = c.h;
    const swplan::ScanPlan& p = c.plan;
    int rc;
    h->had_intra = true;
    HIPCHECK(mark(h, 6, h->stream.get()));
    const sw_db::LptTable* t = lpt_table(c.db, p);
    if (!t) return SW_E_HIP;
    swk::IntraArgs x = c.x;
    x.pipe_pairs = t->npipe;
    x.pipe_tail = t->pipe_tail;
    const swk::DrainArgs* dargs = nullptr;
    if (p.drain && (rc = drain_args(c, x, *t, &dargs))) return rc;
    HIPCHECK(swk::launch_scan_lpt(c.a, x, t->d_order.get(), t->n, p.affine, p.ri2, h->cus, h->stream.get(), dargs,
                                  c.lpt_next, h->opts.lpt_persist >= 2 ? h->opts.lpt_persist : 0, p.lpt_rows));
    ++h->launches;
    // (a draining launch ends the scan: its end event is ev[3])
    if (!p.drain) HIPCHECK(mark(h, 7, h->stream.get()));
    // the fp16 pass's flagged count, as long_pass's
    if ((rc = readback_record(c.db->lcount, {c.skey, c.qhash, c.qlen, 0}, c.list1, nullptr, h->stream.get()))) return rc;
    if (!p.drain && (rc = intra_tail(c, h->stream.get()))) return rc;
    return inter_tail(c);
}

// A deferred scan's rescue tail beside the next scan's fp16 passes.
int deferred_tails(Scan& c) {
    sw_handle* h = c.h;
    int rc;
    if (!c.deferred || !(c.inter_tail || c.intra_tail)) return SW_OK;
    const RescueStages s = rescue_stages(c, c.x, tail_rows(c.db->lay), false);
    if (c.inter_tail) {
        HIPCHECK(hipStreamWaitEvent(h->tail.get(), h->main_done.get(), 0));
        if ((rc = launch_inter_tail(c, h->tail.get(), s))) return rc;
    }
    if (c.intra_tail) {
        HIPCHECK(hipStreamWaitEvent(h->tail.get(), h->side_done.get(), 0));
        if ((rc = launch_intra_tail(c, h->tail.get(), s))) return rc;
    }
    HIPCHECK(hipEventRecord(h->tail_done[c.par].get(), h->tail.get()));
    h->tail_pending[c.par] = true;
    sw_handle::ProfSlot& S = h->prof[c.P.slot];
    HIPCHECK(hipEventRecord(S.tail_read.get(), h->tail.get()));
    S.tail_pending = true;
    return SW_OK;
}

// sw_opts rescue_stats: what the guard bands flagged (synchronises).
int print_rescue_stats(const Scan& c) {
    sw_handle* h = c.h;
    const sw_db* db = c.db;
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->tail.get()));
    int32_t cA = 0, cB = 0, l1 = 0, l2 = 0;
    std::vector<int32_t> ids;
    if (c.listA) {
        HIPCHECK(hipMemcpy(&cA, c.listA, 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(&cB, c.listB, 4, hipMemcpyDeviceToHost));
        ids.resize(static_cast<size_t>(cA));
        if (cA) HIPCHECK(hipMemcpy(ids.data(), c.listA + 1, 4 * ids.size(), hipMemcpyDeviceToHost));
    }
    if (c.list1) {
        HIPCHECK(hipMemcpy(&l1, c.list1, 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(&l2, c.list2, 4, hipMemcpyDeviceToHost));
    }
    int64_t res = 0;
    int32_t wmin = 1 << 30, wmax = 0, bmin = 1 << 30, bmax = -1;
    for (int32_t b : ids) {
        if (b < 0) continue;  // (taken entries are reset to -1: a drained list shows counts only)
        res += db->shape.blk_res[b];
        wmin = std::min<int32_t>(wmin, db->shape.blk_groups[b] * 16);
        wmax = std::max<int32_t>(wmax, db->shape.blk_groups[b] * 16);
        bmin = std::min(bmin, b);
        bmax = std::max(bmax, b);
    }
    std::fprintf(stderr,
                 "rescue: qlen %d go %d ge %d: inter %d/%lld blocks flagged (ids %d..%d, widths %d..%d, "
                 "%lld of %lld residues), %d again; pairs %d; intra %d/%lld flagged, %d again\n",
                 c.qlen, c.sc.go, c.sc.ge, cA, static_cast<long long>(db->shape.nblocks), bmin, bmax, wmin, wmax,
                 static_cast<long long>(res), static_cast<long long>(db->residues), cB, c.plan.npair, l1,
                 static_cast<long long>(db->shape.nlong), l2);
    return SW_OK;
}

// One scan (swd::scan_impl states the arguments).  The two forms of src differ
// in the scoring's checks and keys here and in scan_profiles; everything else
// is one path.
int scan_impl_body(sw_handle* h, const sw_db* cdb, const QuerySrc& src, int32_t* scores_dev, bool defer,
                   const RankReq* rq, uint32_t* hist) {
    sw_db* db = mutable_db(cdb);
    const uint8_t* query = src.codes;
    const int32_t qlen = src.qlen;
    if (!h || !db || (!src.pssm && !query && qlen > 0) || qlen < 0 || !scores_dev)
        return fail(SW_E_INVALID, "null argument");
    if (rq || hist) defer = false;  // the ranking and the table read every rescued score
    const int8_t* mat = nullptr;
    int go = src.go, ge = src.ge, rc;
    if (src.pssm && (rc = check_pssm(h, src.pssm, go, ge))) return rc;
    if ((rc = check_fault(h))) return rc;
    if (!src.pssm && (rc = check_scoring(src.sc, &mat, &go, &ge))) return rc;
    if (!db->lay.built && (rc = build_db(db))) return rc;
    HIPCHECK(hipSetDevice(h->device));
    h->launches = 0;
    h->had_intra = false;
    if ((rc = next_events(h))) return rc;
    if (qlen == 0) return scan_empty(h, db, scores_dev, defer, rq, hist);

    Scan c;
    c.h = h;
    c.db = db;
    c.qlen = qlen;
    c.scores = scores_dev;
    // The adaptive state's keys.  Bit 63 of skey is the form's tag: clear for
    // a matrix scoring, set for a PSSM's (its gaps alone; the table is the
    // "query", qhash), so a PSSM scan and a sequence scan of the same length
    // never share an observation.
    constexpr uint64_t kPssmTag = 1ull << 63;
    c.skey = 1469598103934665603ull;
    if (src.pssm) {
        c.sc = swplan::plan_scoring_max(src.pssm->max_entry, go, ge);
        c.qhash = src.pssm->hash;
    } else {
        c.sc = swplan::plan_scoring(mat, go, ge);
        for (int k = 0; k < 625; ++k) c.skey = (c.skey ^ static_cast<uint8_t>(mat[k])) * 1099511628211ull;
        c.qhash = 1469598103934665603ull;
        for (int32_t k = 0; k < qlen; ++k) c.qhash = (c.qhash ^ query[k]) * 1099511628211ull;
    }
    c.skey = ((c.skey ^ static_cast<uint32_t>(go)) * 1099511628211ull ^ static_cast<uint32_t>(ge)) * 1099511628211ull;
    c.skey = src.pssm ? c.skey | kPssmTag : c.skey & ~kPssmTag;

    // The form of the scan: the two adaptive routes from the database's
    // earlier scans, then the plan; a merged launch drains its own rescue
    // lists when it gets boundary rows for that.
    const bool i16_first = adapt_intra_i16_first(db, c.skey, qlen, h->opts.intra_i16_first);
    const int32_t i16_span = adapt_inter_i16_span(db, c.skey, qlen, h->opts.inter_i16_span);
    c.plan = swplan::scan_plan(plan_view(db), qlen, c.sc, i16_first, i16_span);
    if (c.plan.lpt) c.plan.set_drain(ensure_rbnd(db, c.plan.affine, c.plan.intra_x2));
    const swplan::ScanPlan& p = c.plan;
    db->last_ncoop = p.ncoop;
    db->last_npair = p.npair;
    db->last_pair_merged = p.npair != 0;

    if ((rc = scan_lists(c, defer))) return rc;
    if ((rc = scan_profiles(c, src, mat))) return rc;
    if ((rc = scan_args(c))) return rc;
    if (!p.kernel.empty()) h->last_kernel = p.kernel;
    h->last_intra = p.intra_kernel;
    if (p.lpt) {
        if ((rc = merged_pass(c))) return rc;
    } else {
        // fork: the side streams start when the main stream reaches ev[0]
        // (the merged launch has none: its scan time runs from ev[6])
        HIPCHECK(mark(h, 0, h->stream.get()));
        if (db->shape.nlong && (rc = long_pass(c))) return rc;
        HIPCHECK(mark(h, 1, db->shape.nlong ? h->side.get() : h->stream.get()));
        if (db->shape.nblocks && (rc = inter_pass(c))) return rc;
    }
    if ((rc = deferred_tails(c))) return rc;

    // join (the merged launch has no separate inter end, nor a side stream
    // to join), rank, and the end event
    if (!db->shape.nblocks)
        for (int k = 6; k < 8; ++k) HIPCHECK(mark(h, k, h->stream.get()));
    if (!p.lpt) HIPCHECK(mark(h, 2, h->stream.get()));
    if (db->shape.nlong && !p.lpt) HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->ev[1].get(), 0));
    // the scan completes on the handle's stream: so do earlier deferred tails
    if (!c.deferred && (rc = join_tails(h))) return rc;
    if (rq && (rc = rank_after(h, db, scores_dev, *rq))) return rc;
    if (hist && (rc = hist_after(h, db, scores_dev, hist))) return rc;
    HIPCHECK(mark(h, 3, h->stream.get()));
    h->open_slot = -1;
    h->evpool[h->nscans - 1].launches = h->launches;
    h->timed = true;
    return h->opts.rescue_stats == 1 ? print_rescue_stats(c) : SW_OK;
}

}  // namespace

int swd::check_pssm(const sw_handle* h, const sw_pssm* p, int go, int ge) {
    if (!h || !p) return fail(SW_E_INVALID, "null argument");
    if (p->h->device != h->device) return fail(SW_E_INVALID, "the PSSM was created on another handle's device");
    return check_gaps(go, ge);
}

int swd::check_batch(const int64_t* qoffsets, int32_t nq) {
    if (nq > 0 && qoffsets[0] < 0) return fail(SW_E_INVALID, "bad query offsets");
    for (int32_t k = 0; k < nq; ++k) {
        const int64_t ql = qoffsets[k + 1] - qoffsets[k];
        if (ql < 0 || ql > (int64_t(1) << 24)) return fail(SW_E_INVALID, "bad query offsets");
    }
    return SW_OK;
}

// A new workspace starts with the one-launch top-K's counter at zero
// (swk::launch_topk).
int swd::ensure_topk_work(sw_handle* h, size_t need) {
    if (need > h->topk_cap) {
        if (h->d_topk_work.get()) {
            HIPCHECK(hipStreamSynchronize(h->stream.get()));
            h->d_topk_work.reset();
        }
        h->topk_cap = 0;
        const size_t cap = std::max<size_t>(need, 1 << 20);
        HIPCHECK(swk::dev_alloc(h->d_topk_work, cap));
        h->topk_cap = cap;
        HIPCHECK(hipMemsetAsync(h->d_topk_work.get(), 0, 256, h->stream.get()));
    }
    return SW_OK;
}

// The calibration table of a score array over a database's subjects
// (sw_calib.hip): the table zeroed, then one count per subject, on the
// handle's stream.
int swd::hist_after(sw_handle* h, sw_db* db, const int32_t* scores_dev, uint32_t* hist_dev) {
    HIPCHECK(hipMemsetAsync(hist_dev, 0, swcalib::kCells * sizeof(uint32_t), h->stream.get()));
    if (db->n == 0) return SW_OK;
    const int32_t *rid = nullptr, *slen = nullptr;
    int rc;
    if ((rc = subject_ids(db, &rid))) return rc;
    if ((rc = subject_lengths(db, &slen))) return rc;
    HIPCHECK(swk::launch_score_hist(scores_dev, rid, slen, db->n, hist_dev, h->stream.get()));
    ++h->launches;
    return SW_OK;
}

// A scan that fails after its profiles were built leaves the profile slot
// pending on an end event it never recorded: a later scan reusing the slot
// would not wait for the kernels this one queued.  Drain the handle's streams
// and release the slot instead.
int swd::scan_impl(sw_handle* h, const sw_db* db, const QuerySrc& src, int32_t* scores_dev, bool defer,
                   const RankReq* rq, uint32_t* hist) {
    const int rc = scan_impl_body(h, db, src, scores_dev, defer, rq, hist);
    if (h && h->open_slot >= 0) {
        (void)quiesce(h);
        h->prof[h->open_slot].pending = false;
        h->open_slot = -1;
    }
    return rc;
}

// ===========================================================================
extern "C" {

// 0.2: sw_pssm_*; 0.3: sw_hit_stats, sw_scan_hits; 0.4: sw_scan_batch_topk, sw_*_hits batch forms;
// 0.5: sw_score_hist*, sw_calib_*, the _sig and _calib scan forms; 0.6: sw_sig_*, the _ranked scan forms
int32_t sw_version(void) { return 10000 * 0 + 100 * 7 + 0; }

#ifndef SW_SOURCE_ID
#define SW_SOURCE_ID "unknown"
#endif
const char* sw_build_id(void) { return SW_SOURCE_ID; }

int sw_scan_device(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                   int32_t* scores_dev) {
    return scan_impl(h, db, seq_src(query, qlen, sc), scores_dev);
}

int sw_scan_pssm_device(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                        int32_t* scores_dev) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return scan_impl(h, db, pssm_src(p, gap_open, gap_extend), scores_dev);
}

int sw_scan_batch_device(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                         const sw_scoring* sc, int32_t* scores_dev) {
    if (!h || !db || nq < 0 || (nq > 0 && (!qoffsets || !queries || !scores_dev)))
        return fail(SW_E_INVALID, "null argument");
    int rc;
    if ((rc = check_batch(qoffsets, nq))) return rc;
    const size_t n = static_cast<size_t>(db->max_id + 1);
    // back to back on the handle's stream: no host synchronisation between
    // queries (profiles go through the slot ring), so the GPU never idles
    // ... and each query's rescue tail runs beside the next query's passes,
    // when a later non-empty query (a real scan, which joins the tails) follows
    int32_t last_scan = -1;
    for (int32_t k = 0; k < nq; ++k)
        if (qoffsets[k + 1] > qoffsets[k]) last_scan = k;
    for (int32_t k = 0; k < nq; ++k)
        if ((rc = scan_impl(h, db, seq_src(queries + qoffsets[k], static_cast<int32_t>(qoffsets[k + 1] - qoffsets[k]), sc),
                            scores_dev + k * n, k < last_scan)))
            return rc;
    // every tail has joined the handle's stream by now; join again in case a
    // scan above fell back to stream order after deferring an earlier one
    HIPCHECK(hipSetDevice(h->device));
    return join_tails(h);
}

int sw_scan_rank_device(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                        int32_t* scores_dev, int32_t k, const int32_t* gid_dev, int64_t id_base,
                        int64_t* keys_out_dev) {
    if (!h || !db || !scores_dev || !keys_out_dev || k <= 0 || k > 4096)
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (!gid_dev && (id_base < 0 || id_base + db->max_id >= (int64_t(1) << 31)))
        return fail(SW_E_INVALID, "ids must fit in 31 bits");
    const RankReq rq{k, gid_dev, gid_dev ? 0 : id_base, keys_out_dev};
    return scan_impl(h, db, seq_src(query, qlen, sc), scores_dev, false, &rq);
}

}  // extern "C"
