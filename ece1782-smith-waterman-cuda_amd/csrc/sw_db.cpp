// sw_db.cpp — a database of the host driver (sw_driver.h): its lifetime, the
// device half of packing (the layout's shape is sw_pack.cpp's), the arrays a
// scan asks for on first need (boundary rows, result ids, lengths), and the
// two lookups from a result id to where the subject is resident.
//
// What the reference does per query (SWSolver.cu:301-371), re-packing the
// whole database into managed memory longest-first, 32 lanes per block,
// happens ONCE here: sw_db_create packs into 64-lane blocks of 16-residue
// groups, sorted longest-first, and keeps the result resident in HBM.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <new>

#include "sw_dbfile.h"
#include "sw_driver.h"
#include "sw_parallel.h"
#include "sw_synth_host.h"

using namespace swd;
using swk::parallel_for;

namespace {

// sw_db_reset_adaptive: forget what earlier scans observed.
void reset_adaptive(sw_db* db) {
    db->lcount.reset();
    db->i16_first.clear();
    db->icount.reset();
    db->i16_span.clear();
}

// Release the packed layout (the caller has quiesced the handle) and forget
// what earlier scans observed on it.
void free_dev(sw_db* db) {
    db->lay = sw_db::Layout{};
    reset_adaptive(db);  // the long partition and the block layout may change
}

template <class T>
int upload(DevPtr<T>& d, const std::vector<T>& v, hipStream_t s, size_t* acc) {
    if (v.empty()) return SW_OK;
    HIPCHECK(swk::dev_alloc(d, v.size() * sizeof(T)));
    HIPCHECK(hipMemcpyAsync(d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    *acc += v.size() * sizeof(T);
    return SW_OK;
}

// Upload bytes produced unit by unit (unit u covers [bounds[u], bounds[u+1])
// of `dev` and fill(u, dst) writes all of it, padding included) through the
// handle's two pinned staging buffers: chunks of whole units are packed on
// the host's cores into one buffer while the previous chunk's H2D copy runs
// (the reference packs byte by byte into managed memory on one thread,
// SWSolver.cu:309-359).
constexpr size_t kStageBytes = size_t(32) << 20;

template <class F>
int staged_upload(sw_handle* h, uint8_t* dev, const std::vector<uint64_t>& bounds, F&& fill) {
    const int64_t nu = static_cast<int64_t>(bounds.size()) - 1;
    if (nu <= 0 || bounds.back() == bounds.front()) return SW_OK;
    uint64_t maxu = 0;
    for (int64_t u = 0; u < nu; ++u) maxu = std::max<uint64_t>(maxu, bounds[u + 1] - bounds[u]);
    const size_t cap = std::max<size_t>(kStageBytes, maxu);
    if (cap > h->stage_cap) {
        for (int b = 0; b < 2; ++b) {
            if (h->stage_pending[b]) HIPCHECK(hipEventSynchronize(h->stage_ev[b].get()));
            h->stage_pending[b] = false;
            h->stage[b].reset();
        }
        h->stage_cap = 0;
        for (int b = 0; b < 2; ++b)
            HIPCHECK(swk::host_alloc(h->stage[b], cap, hipHostMallocDefault));
        h->stage_cap = cap;
    }
    int b = 0;
    for (int64_t u0 = 0; u0 < nu;) {
        int64_t u1 = u0 + 1;
        while (u1 < nu && bounds[u1 + 1] - bounds[u0] <= h->stage_cap) ++u1;
        if (h->stage_pending[b]) HIPCHECK(hipEventSynchronize(h->stage_ev[b].get()));
        uint8_t* buf = h->stage[b].get();
        const uint64_t base = bounds[u0];
        parallel_for(u1 - u0, [&](int64_t i) { fill(u0 + i, buf + (bounds[u0 + i] - base)); }, 1);
        HIPCHECK(hipMemcpyAsync(dev + base, buf, bounds[u1] - base, hipMemcpyHostToDevice, h->stream.get()));
        HIPCHECK(hipEventRecord(h->stage_ev[b].get(), h->stream.get()));
        h->stage_pending[b] = true;
        b ^= 1;
        u0 = u1;
    }
    return SW_OK;
}

// The subjects as the packer reads them (sw_pack.h).
swpack::Subjects subjects_view(const sw_db* db) {
    swpack::Subjects v;
    v.n = db->n;
    v.offsets = db->h_offsets.data();
    v.ids = db->h_ids.data();
    v.residues = db->synthetic ? nullptr : db->h_residues.data();
    return v;
}

}  // namespace

swplan::PlanDb swd::plan_view(const sw_db* db) {
    swplan::PlanDb v;
    v.n = db->n;
    v.residues = db->residues;
    v.nblocks = db->shape.nblocks;
    v.nlong = db->shape.nlong;
    v.long_threshold = db->long_threshold;
    v.long_max = db->shape.long_max;
    v.blk_groups = db->shape.blk_groups.data();
    v.llen = db->shape.llen.data();
    v.opts = &db->h->opts;
    v.cus = db->h->cus;
    return v;
}

void swd::subject_residues(const sw_db* db, int64_t k, uint8_t* out) {
    const int64_t L = db->h_offsets[k + 1] - db->h_offsets[k];
    if (db->synthetic)
        swk::synth_residues(db->seed, static_cast<uint64_t>(db->id_base + db->h_ids[k]), L, out);
    else
        std::memcpy(out, db->h_residues.data() + db->h_offsets[k], L);
}

// The device half of packing: the layout's shape is sw_pack.cpp's; allocate
// it, upload the residues as the packer fills them (or generate them in
// place), upload its tables, and keep the shape.
int swd::build_db(sw_db* db) {
    hipStream_t s = db->h->stream.get();
    const swpack::Subjects subj = subjects_view(db);
    swpack::Shape sh = swpack::plan(subj, db->long_threshold, db->synthetic);
    const uint64_t total = sh.total, ltotal = sh.ltotal;

    size_t acc = 0;
    int rc;
    if (db->synthetic) {
        // residues generated in HBM from (seed, global id); ids in lane_ids
        // and lid are local (0..n-1), global = id_base + local
        if (total) HIPCHECK(swk::dev_alloc(db->lay.d_res, total));
        if (ltotal) HIPCHECK(swk::dev_alloc(db->lay.d_lres, ltotal));
        acc += total + ltotal;
    } else {
        // residues through pinned staging, packed in parallel chunks
        if (total) {
            HIPCHECK(swk::dev_alloc(db->lay.d_res, total));
            if ((rc = staged_upload(db->h, db->lay.d_res.get(), sh.blk_off,
                                    [&](int64_t b, uint8_t* dst) { swpack::fill_block(subj, sh, b, dst); })))
                return rc;
        }
        if (ltotal) {
            HIPCHECK(swk::dev_alloc(db->lay.d_lres, ltotal));
            if ((rc = staged_upload(db->h, db->lay.d_lres.get(), sh.loff,
                                    [&](int64_t k, uint8_t* dst) { swpack::fill_long(subj, sh, k, dst); })))
                return rc;
        }
        acc += total + ltotal;
    }
    sh.blk_off.pop_back();  // the kernels' tables have no end entry
    sh.loff.pop_back();
    if ((rc = upload(db->lay.d_blk_off, sh.blk_off, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_blk_groups, sh.blk_groups, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_blk_cols, sh.blk_cols, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_lane_ids, sh.lane_ids, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_loff, sh.loff, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_llen, sh.llen, s, &acc))) return rc;
    if ((rc = upload(db->lay.d_lid, sh.lid, s, &acc))) return rc;
    if (db->synthetic) {
        DevPtr<int32_t> d_lane_len;  // the fill's inputs, released after it has run
        DevPtr<uint8_t> d_lut;
        size_t tmp = 0;
        if ((rc = upload(d_lane_len, sh.lane_len, s, &tmp))) return rc;
        const swk::SynthTables& T = swk::synth_tables();
        HIPCHECK(swk::dev_alloc(d_lut, sizeof T.lut_stored));
        HIPCHECK(hipMemcpyAsync(d_lut.get(), T.lut_stored, sizeof T.lut_stored, hipMemcpyHostToDevice, s));
        swk::SynthFill f{};
        f.res = db->lay.d_res.get();
        f.blk_off = db->lay.d_blk_off.get();
        f.blk_groups = db->lay.d_blk_groups.get();
        f.lane_local = db->lay.d_lane_ids.get();
        f.lane_len = d_lane_len.get();
        f.nblocks = sh.nblocks;
        f.lres = db->lay.d_lres.get();
        f.loff = db->lay.d_loff.get();
        f.llen = db->lay.d_llen.get();
        f.lid = db->lay.d_lid.get();
        f.nlong = static_cast<int32_t>(sh.nlong);
        f.seed = db->seed;
        f.id_base = db->id_base;
        f.lut = d_lut.get();
        HIPCHECK(swk::launch_synth_fill(f, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    HIPCHECK(hipStreamSynchronize(s));  // the uploads' sources go away
    sh.release_upload_tables();
    db->shape = std::move(sh);
    db->lay.device_bytes = acc;
    db->lay.built = true;
    return SW_OK;
}

// Boundary rows are only needed when the query spans more than one strip;
// allocate on first need and keep.
int swd::ensure_bnd(sw_db* db, bool affine, bool intra_f) {
    const size_t res = db->shape.total * 4, lres = db->shape.ltotal * 4;
    const struct {
        DevPtr<int32_t>& p;
        size_t bytes;
    } rows[] = {{db->lay.d_bnd_h, res}, {db->lay.d_bnd_f, affine ? res : 0},
                {db->lay.d_lbnd_h, lres}, {db->lay.d_lbnd_f, (affine || intra_f) ? lres : 0}};
    for (const auto& r : rows)
        if (r.bytes && !r.p.get()) {
            HIPCHECK(swk::dev_alloc(r.p, r.bytes));
            db->lay.device_bytes += r.bytes;
        }
    return SW_OK;
}

// The deferred tails' own boundary rows, sized as ensure_bnd's: H always, F
// only for affine scoring (inter) or when the intra form keeps F (intra_f).
// Arrays a later scan needs are allocated then.  False when device memory
// would drop below a quarter of the card's (a 50M-subject database keeps its
// tails in stream order); a refused size is not tried again for this layout.
bool swd::ensure_rbnd(sw_db* db, bool affine, bool intra_f) {
    DevPtr<int32_t>* const p[4] = {&db->lay.d_rbnd_h, &db->lay.d_rbnd_f, &db->lay.d_rlbnd_h, &db->lay.d_rlbnd_f};
    const size_t sz[4] = {db->shape.total * 4, affine ? db->shape.total * 4 : 0, db->shape.ltotal * 4,
                          (affine || intra_f) ? db->shape.ltotal * 4 : 0};
    size_t need = 0;
    for (int k = 0; k < 4; ++k)
        if (sz[k] && !p[k]->get()) need += sz[k];
    if (need == 0) return true;
    if (db->lay.rbnd_tried) return false;
    size_t freeb = 0, totalb = 0;
    if (hipMemGetInfo(&freeb, &totalb) != hipSuccess || freeb < need + totalb / 4) {
        db->lay.rbnd_tried = true;
        return false;
    }
    for (int k = 0; k < 4; ++k)
        if (sz[k] && !p[k]->get()) {
            if (swk::dev_alloc(*p[k], sz[k]) != hipSuccess) {
                (void)hipGetLastError();
                db->lay.rbnd_tried = true;
                return false;
            }
            db->lay.device_bytes += sz[k];
        }
    return true;
}

int swd::subject_ids(sw_db* db, const int32_t** rid) {
    if (db->rid_identity < 0) {
        db->rid_identity = db->max_id + 1 == db->n;
        for (int64_t k = 0; db->rid_identity == 1 && k < db->n; ++k) db->rid_identity = db->h_ids[k] == k;
    }
    *rid = nullptr;
    if (!db->rid_identity) {
        if (!db->lay.d_ids.get()) {
            HIPCHECK(swk::dev_alloc(db->lay.d_ids, static_cast<size_t>(db->n) * sizeof(int32_t)));
            HIPCHECK(hipMemcpy(db->lay.d_ids.get(), db->h_ids.data(), static_cast<size_t>(db->n) * sizeof(int32_t),
                               hipMemcpyHostToDevice));
            db->lay.device_bytes += static_cast<size_t>(db->n) * sizeof(int32_t);
        }
        *rid = db->lay.d_ids.get();
    }
    return SW_OK;
}

// (beside d_ids: whatever the long threshold is, the order is the same)
int swd::subject_lengths(sw_db* db, const int32_t** slen) {
    if (!db->lay.d_slen.get()) {
        std::vector<int32_t> L(static_cast<size_t>(db->n));
        for (int64_t k = 0; k < db->n; ++k) L[k] = static_cast<int32_t>(db->h_offsets[k + 1] - db->h_offsets[k]);
        HIPCHECK(swk::dev_alloc(db->lay.d_slen, L.size() * sizeof(int32_t)));
        HIPCHECK(hipMemcpy(db->lay.d_slen.get(), L.data(), L.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        db->lay.device_bytes += L.size() * sizeof(int32_t);
    }
    *slen = db->lay.d_slen.get();
    return SW_OK;
}

int64_t swd::subject_of(sw_db* db, int32_t id) {
    if (db->id_index.empty())
        for (int64_t k = 0; k < db->n; ++k) db->id_index.emplace(db->h_ids[k], k);
    const auto it = db->id_index.find(id);
    return it == db->id_index.end() ? -1 : it->second;
}

int64_t swd::position_of(sw_db* db, int64_t subj) {
    if (db->pos_of.empty()) {
        const std::vector<int64_t> order = swpack::length_order(db->h_offsets.data(), db->n);
        db->pos_of.resize(static_cast<size_t>(db->n));
        for (int64_t p = 0; p < db->n; ++p) db->pos_of[order[p]] = p;
    }
    return db->pos_of[subj];
}

extern "C" {

int sw_db_create(sw_handle* h, const uint8_t* residues, const int64_t* offsets, int64_t n, const int32_t* ids,
                 sw_db** out) {
    if (!h || !out || n < 0 || (n > 0 && !offsets)) return fail(SW_E_INVALID, "null argument");
    *out = nullptr;
    if (n > 0 && offsets[0] != 0) return fail(SW_E_INVALID, "offsets[0] must be 0");
    for (int64_t k = 0; k < n; ++k)
        if (offsets[k + 1] < offsets[k]) return fail(SW_E_INVALID, "offsets must be non-decreasing");
    const int64_t total = n > 0 ? offsets[n] : 0;
    if (total > 0 && !residues) return fail(SW_E_INVALID, "null residues");
    for (int64_t k = 0; k < n; ++k)
        if (offsets[k + 1] - offsets[k] > (int64_t(1) << 30)) return fail(SW_E_INVALID, "subject too long");
    std::unique_ptr<sw_db> db(new (std::nothrow) sw_db());
    if (!db) return fail(SW_E_NOMEM, "out of host memory");
    db->h = h;
    db->n = n;
    try {
        db->h_residues.resize(static_cast<size_t>(total));
        db->h_offsets.assign(offsets, offsets + n + 1);
        if (n == 0) db->h_offsets.assign(1, 0);
        db->h_ids.resize(n);
        for (int64_t k = 0; k < n; ++k) db->h_ids[k] = ids ? ids[k] : static_cast<int32_t>(k);
    } catch (...) {
        return fail(SW_E_NOMEM, "out of host memory");
    }
    // copy and validate in parallel 1 MiB pieces
    constexpr int64_t kPiece = int64_t(1) << 20;
    std::atomic<bool> bad{false};
    parallel_for((total + kPiece - 1) / kPiece, [&](int64_t c) {
        const int64_t lo = c * kPiece, hi = std::min(total, lo + kPiece);
        std::memcpy(db->h_residues.data() + lo, residues + lo, static_cast<size_t>(hi - lo));
        uint8_t m = 0;
        for (int64_t k = lo; k < hi; ++k) m = std::max(m, residues[k]);
        if (m >= SW_ALPHABET) bad = true;
    }, 1);
    if (bad) return fail(SW_E_INVALID, "residue code out of range (use sw_encode)");
    db->residues = total;
    for (int64_t k = 0; k < n; ++k) {
        db->max_len = std::max<int32_t>(db->max_len, static_cast<int32_t>(offsets[k + 1] - offsets[k]));
        if (db->h_ids[k] < 0) return fail(SW_E_INVALID, "ids must be >= 0");
        db->max_id = std::max(db->max_id, db->h_ids[k]);
    }
    db->long_threshold = swplan::default_long_threshold(plan_view(db.get()));
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = build_db(db.get())) return rc;
    *out = db.release();
    return SW_OK;
}

// ---- binary database file (sw_dbfile.cpp) ----------------------------------
int sw_db_save(const sw_db* db, const char* path) {
    if (!db || !path) return fail(SW_E_INVALID, "null argument");
    // length-sorted (descending, stable), ids kept: loading gives identical scores[id]
    const int64_t n = db->n;
    const std::vector<int64_t> order = swpack::length_order(db->h_offsets.data(), n);
    auto len = [&](int64_t k) { return db->h_offsets[k + 1] - db->h_offsets[k]; };
    std::vector<int64_t> offs(n + 1, 0);
    std::vector<int32_t> ids(n);
    std::vector<uint8_t> res(static_cast<size_t>(db->residues));
    for (int64_t k = 0; k < n; ++k) {
        const int64_t src = order[k];
        subject_residues(db, src, res.data() + offs[k]);
        offs[k + 1] = offs[k] + len(src);
        ids[k] = db->h_ids[src];
    }
    return swdbfile::write(path, offs, ids, res, db->max_len);
}

int sw_db_load(sw_handle* h, const char* path, sw_db** out) {
    if (!h || !path || !out) return fail(SW_E_INVALID, "null argument");
    *out = nullptr;
    std::vector<int64_t> offs;
    std::vector<int32_t> ids;
    std::vector<uint8_t> res;
    if (int rc = swdbfile::read(path, offs, ids, res)) return rc;
    return sw_db_create(h, res.data(), offs.data(), static_cast<int64_t>(ids.size()), ids.data(), out);
}

int sw_synth_tables(int32_t* len4096, uint8_t* lut65536) {
    const swk::SynthTables& T = swk::synth_tables();
    if (len4096) std::memcpy(len4096, T.len, sizeof T.len);
    if (lut65536) std::memcpy(lut65536, T.lut, sizeof T.lut);
    return SW_OK;
}

int sw_synth_lengths(uint64_t seed, int64_t id_base, int64_t n, int32_t* lengths) {
    if (n < 0 || (n > 0 && !lengths) || id_base < 0) return fail(SW_E_INVALID, "null argument");
    parallel_for(n, [&](int64_t k) { lengths[k] = swk::synth_length(seed, static_cast<uint64_t>(id_base + k)); });
    return SW_OK;
}

int sw_db_create_synthetic(sw_handle* h, uint64_t seed, int64_t id_base, int64_t n, sw_db** out) {
    if (!h || !out || n < 0 || id_base < 0 || n > (int64_t(1) << 31) - 1) return fail(SW_E_INVALID, "bad argument");
    *out = nullptr;
    std::unique_ptr<sw_db> db(new (std::nothrow) sw_db());
    if (!db) return fail(SW_E_NOMEM, "out of host memory");
    db->h = h;
    db->n = n;
    db->synthetic = true;
    db->seed = seed;
    db->id_base = id_base;
    try {
        std::vector<int32_t> L(n);
        sw_synth_lengths(seed, id_base, n, L.data());
        db->h_offsets.assign(n + 1, 0);
        for (int64_t k = 0; k < n; ++k) db->h_offsets[k + 1] = db->h_offsets[k] + L[k];
        db->h_ids.resize(n);
        for (int64_t k = 0; k < n; ++k) db->h_ids[k] = static_cast<int32_t>(k);
        for (int64_t k = 0; k < n; ++k) db->max_len = std::max(db->max_len, L[k]);
    } catch (...) {
        return fail(SW_E_NOMEM, "out of host memory");
    }
    db->residues = db->h_offsets[n];
    db->max_id = static_cast<int32_t>(n - 1);
    db->long_threshold = swplan::default_long_threshold(plan_view(db.get()));
    HIPCHECK(hipSetDevice(h->device));
    if (int rc = build_db(db.get())) return rc;
    *out = db.release();
    return SW_OK;
}

int sw_db_subjects(const sw_db* db, int64_t* lengths, int32_t* ids) {
    if (!db) return fail(SW_E_INVALID, "null argument");
    for (int64_t k = 0; k < db->n; ++k) {
        if (lengths) lengths[k] = db->h_offsets[k + 1] - db->h_offsets[k];
        if (ids) ids[k] = db->h_ids[k];
    }
    return SW_OK;
}

int sw_db_free(sw_db* db) {
    if (!db) return SW_OK;
    (void)hipSetDevice(db->h->device);
    (void)quiesce(db->h);
    if (db->lay.h_trace.get()) {  // the last scan's block timeline (tail analysis builds)
        if (const char* path = db->h->opts.trace_file; path[0])
            if (FILE* f = std::fopen(path, "wb")) {
                std::fwrite(db->lay.h_trace.get(), 32, db->lay.trace_entries, f);
                std::fclose(f);
            }
    }
    delete db;
    return SW_OK;
}

int sw_db_reset_adaptive(sw_db* db) {
    if (!db) return fail(SW_E_INVALID, "null argument");
    reset_adaptive(db);
    return SW_OK;
}

int sw_db_get_stats(const sw_db* db, sw_db_stats* out) {
    if (!db || !out) return fail(SW_E_INVALID, "null argument");
    out->n_subjects = db->n;
    out->residues = db->residues;
    out->packed_cells = static_cast<int64_t>(db->shape.total);  // one byte per scanned (lane, column)
    out->n_blocks = db->shape.nblocks;
    out->n_long = db->shape.nlong;
    out->device_bytes = static_cast<int64_t>(db->lay.device_bytes);
    out->max_length = db->max_len;
    out->long_threshold = db->long_threshold;
    out->coop_blocks = db->lay.built ? db->last_ncoop : 0;
    out->coop_residues = 0;
    for (int32_t b = 0; b < out->coop_blocks; ++b) out->coop_residues += db->shape.blk_res[b];
    out->pair_blocks = db->lay.built ? db->last_npair : 0;
    out->pair_merged = db->lay.built && db->last_pair_merged ? 1 : 0;
    out->pair_residues = 0;
    for (int32_t b = 0; b < out->pair_blocks; ++b) out->pair_residues += db->shape.blk_res[b];
    out->max_id = db->max_id;
    return SW_OK;
}

int sw_db_set_long_threshold(sw_db* db, int32_t threshold) {
    if (!db) return fail(SW_E_INVALID, "null argument");
    if (threshold < 0) return fail(SW_E_INVALID, "threshold must be >= 0");
    const int32_t t = threshold == 0 ? swplan::default_long_threshold(plan_view(db)) : threshold;
    if (t == db->long_threshold && db->lay.built) return SW_OK;
    HIPCHECK(hipSetDevice(db->h->device));
    HIPCHECK(quiesce(db->h));
    free_dev(db);
    db->long_threshold = t;
    return build_db(db);
}

}  // extern "C"
