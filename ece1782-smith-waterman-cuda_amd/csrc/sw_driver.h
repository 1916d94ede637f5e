// sw_driver.h — what the units of the host driver share (internal; the
// library is built -fvisibility=hidden, so nothing here is exported):
//   sw_scoring.cpp  the built-in matrices, the encoder, the scoring checks
//   sw_handle.cpp   the error sink, the handle's streams, events and timing
//   sw_db.cpp       a database's lifetime and device layout
//   sw_capi.cpp     the scan driver: one scan's enqueue, its ranking and table
//   sw_search.cpp   what runs on top of a scan: top-K, hit tables, calibration,
//                   traceback, batches
// The types behind the C ABI's opaque pointers, and the functions that cross
// a unit boundary (namespace swd).  A function only one unit calls is in that
// unit's anonymous namespace, not here.
#pragma once

#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sw_host.h"
#include "sw_pack.h"
#include "sw_plan.h"

namespace swd {

using swk::DevPtr;
using swk::Event;
using swk::HostPtr;
using swk::Stream;

// Record msg as this thread's sw_last_error() and return code.
inline int fail(int code, const std::string& msg) { return swk::set_error(code, msg); }

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// A vector element type that resize() leaves uninitialised (the database's
// host copy is filled by parallel copies right after).
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(p)) U;
        else ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};

struct ScanEvents {
    // 0 fork, 1 intra done (side), 2 inter done (main), 3 end, and around
    // each inter kernel on its own stream: 4/5 the cooperative kernel
    // (side2), 6/7 the per-wave kernel (main)
    Event ev[8];
    unsigned rec = 0;  // bit k: ev[k] was recorded by this scan (read_events
                       // falls back for the others: each record is a packet
                       // the command processor spends microseconds on)
    int launches = 0;
    bool merged = false;  // one merged launch (sw_scan_lpt): ev6..ev7 is the whole scan's fp16 pass
};

// What a scan's fp16 pass flagged, read back without waiting: one or two
// device words copied to a pinned pair in stream order behind the pass, an
// event after the copy, and what the readback observes.  A later scan takes
// it once the event has completed (the adaptive routes, sw_capi.cpp adapt_*);
// a scan repeating the last observation taken does not read it back again.
struct Readback {
    struct Obs {  // scoring key, query hash and length, and (inter) the int16 span the scan ran with
        uint64_t key = 0, qhash = 0;
        int32_t qlen = 0, nr = 0;
        bool operator==(const Obs& o) const { return key == o.key && qhash == o.qhash && qlen == o.qlen && nr == o.nr; }
    };
    HostPtr<int32_t> host;  // pinned [2]
    Event ev;               // both or neither (readback_record)
    bool pending = false;
    bool seen = false;  // `last` holds an observation
    Obs sent, last;     // of the pending readback; of the last one taken
    // Forget the pending and the last observation.  A readback still in
    // flight lands in the same pinned words later, in stream order before any
    // readback a later scan issues: ignoring it is safe.
    void reset() { pending = seen = false; }
};

sw_opts default_opts();  // every override off (sw_handle.cpp)

}  // namespace swd

struct sw_handle {
    int device = 0;
    int cus = 0;  // compute units of the device
    swd::Stream stream;  // the handle's own, or the caller's (sw_set_stream): borrowed, given up
    bool own_stream = false;  // ... before the owner would destroy it
    ~sw_handle() { if (!own_stream) stream.release(); }
    // One event set per scan since the last sw_timing_reset (grows as needed,
    // reused after a reset), so a caller can time many back-to-back scans
    // without synchronising between them.
    std::vector<swd::ScanEvents> evpool;
    size_t nscans = 0;
    swd::Event* ev = nullptr;  // event set of the current scan (an alias into evpool, as ev_rec)
    unsigned* ev_rec = nullptr;
    // The intra kernel runs on a side stream, concurrently with the inter
    // kernel (fork/join through ev[0] and ev[1]).
    swd::Stream side;
    swd::Stream side2;  // the cooperative wide-block kernel
    // Deferred rescue tails (the queries of a batch but the last): a scan's
    // re-scoring stages (int16 / int32 list kernels) run on `tail` after its
    // fp16 passes, while the next query's fp16 passes start on the main and
    // side streams.  Lists and boundary rows of the tail are its own
    // (parity-indexed lists, sw_db::d_rbnd_*), so nothing is shared with the
    // passes running beside it.
    swd::Stream tail;
    swd::Event main_done, side_done;  // fp16 passes of the scan being deferred
    swd::Event tail_done[2];  // per list parity
    bool tail_pending[2] = {};
    int parity = 0;                                       // list set of the next scan
    swd::Event coop_done;
    swd::Event fork2;  // side2 starts after the rescue counters are reset
    // per-query workspace: profiles (inter: [32][stride]; intra: lane-slotted
    // chunks) built on the device by the scan's first launch.  A ring of
    // slots: a deferred rescue tail (batches) may still read the profiles of
    // the scan before while the next scan builds its own.  Reusing a slot
    // waits until the scan that last used it has started on the device, so
    // the host runs at most kProfSlots scans ahead of the GPU: the adaptive
    // choices (the fp16 passes' flagged counts read back without waiting,
    // scan_impl) then see scans a few queries back instead of none at all
    // when many scans are enqueued at once.
    struct ProfSlot {
        swd::DevPtr<int8_t> d;
        size_t dcap = 0;
        // the end event (ev[3]) of the slot's last scan: reusing the slot
        // waits for it.  Not an event of its own: each event record is a
        // packet the command processor spends ~5 us on between two kernels
        // (rocprofv3 trace of C2's 1/8 share, scripts/step_gaps.py)
        hipEvent_t last_end = nullptr;  // (an alias into evpool)
        bool pending = false;
        swd::Event tail_read;  // a deferred rescue tail has read the slot
        bool tail_pending = false;
    };
    // pinned staging of database uploads (build_db): the host packs one
    // buffer while the other's copy runs
    swd::HostPtr<uint8_t> stage[2];
    size_t stage_cap = 0;
    swd::Event stage_ev[2];
    bool stage_pending[2] = {};
    static constexpr int kProfSlots = 4;
    ProfSlot prof[kProfSlots];
    int prof_next = 0;
    swd::DevPtr<int32_t> d_scores;  // for the synchronous sw_scan
    size_t scores_cap = 0;
    swd::DevPtr<int64_t> d_topk_work;  // device top-K workspace
    swd::DevPtr<uint32_t> d_hist;      // the calibration table of the synchronous sw_score_hist
    // pinned landing area of the scans' calibration tables (the _sig and _calib
    // forms): a copy into pageable memory would make the host wait inside
    // hipMemcpyAsync, one more synchronisation in all but name
    swd::HostPtr<uint32_t> h_hist;
    size_t hist_cap = 0;  // ... in tables
    std::string last_kernel = "none";  // per-wave inter kernel of the last scan
    std::string last_intra = "none";   // long-subject kernel of the last scan
    size_t topk_cap = 0;
    bool timed = false;
    bool had_intra = false;
    int launches = 0;
    // host-mapped fault word (swk::DrainArgs::fault): set by a kernel that
    // had to skip work it could not do (list_wait_take's timeout); the next
    // call on the handle fails with SW_E_DEVICE instead of returning scores
    swd::HostPtr<int32_t> h_fault;
    int32_t* d_fault = nullptr;  // the device address of h_fault (an alias)
    int open_slot = -1;  // profile slot pending on an ev[3] this scan has not recorded yet
    sw_opts opts = swd::default_opts();  // kernel-form overrides (sw_set_opts); all -1 = the library's choice
};

struct sw_db {
    sw_handle* h = nullptr;
    int64_t n = 0;
    int64_t residues = 0;
    int32_t max_len = 0;
    int32_t max_id = -1;
    int32_t long_threshold = 0;
    // sw_scan_lpt work tables (longest first), per scan shape
    struct LptTable {
        int32_t qpad, rows /* per pass */, qpad_intra, ri, npair, group /* quad blocks */, tail /* tail-pair blocks */, n;
        bool affine;
        bool tri;  // the group blocks by 3-wave groups with a spare wave (InterArgs::blk_tri)
        int32_t npipe;  // the longest pairs, in the pipelined form
        int32_t pipe_opt;  // sw_opts lpt_pipe the table was built under
        int32_t pipe_tail;  // pairs [pipe_tail, ...) pipelined too (the shortest)
        int32_t tail_opt;   // sw_opts lpt_pipe_tail the table was built under
        swd::DevPtr<int32_t> d_order;
        std::vector<float> cost;  // estimated duration of each entry, longest first
    };
    static constexpr int kDrainSlots = 32;
    // Everything that belongs to one packed layout (one long threshold):
    // build_db and the scans after it fill it, a rebuild replaces it with a
    // fresh one.  What a member of sw_db outside it holds survives a rebuild.
    struct Layout {
        // inter part
        swd::DevPtr<uint8_t> d_res;
        swd::DevPtr<uint64_t> d_blk_off;
        swd::DevPtr<uint32_t> d_blk_groups;
        swd::DevPtr<uint32_t> d_blk_cols;  // block widths rounded to 8 columns (sw_inter_x2s)
        swd::DevPtr<int32_t> d_lane_ids;
        swd::DevPtr<int32_t> d_ids;        // every subject's result id (sw_scan_topk), on first use
        swd::DevPtr<int32_t> d_slen;       // every subject's length, in the same order (sw_score_hist), on first use
        swd::DevPtr<int32_t> d_bnd_h, d_bnd_f;
        // two rescue lists [count, block ids...] of nblocks + 1 ints each: the
        // 16-bit kernels' flagged blocks (list A), and the fp16 chain's second
        // stage's (list B)
        // (two parities of these lists: consecutive scans of a batch alternate)
        swd::DevPtr<int32_t> d_rescue;
        swd::DevPtr<int32_t> d_lrescue;    // [count, subjects...] x 2: the intra rescue chain's lists
        // boundary rows of deferred rescue tails (inter H, F; intra H, F), when
        // device memory allows them (else the tails run in stream order)
        swd::DevPtr<int32_t> d_rbnd_h, d_rbnd_f, d_rlbnd_h, d_rlbnd_f;
        bool rbnd_tried = false;
        // intra part (long subjects)
        swd::DevPtr<uint8_t> d_lres;
        swd::DevPtr<uint64_t> d_loff;
        swd::DevPtr<int32_t> d_llen, d_lid, d_lbnd_h, d_lbnd_f;
        std::vector<LptTable> lpt_tables;
        // device copies of the merged launch's drain arguments (swk::DrainArgs),
        // one per distinct content (profile slot x list parity x score buffer
        // x query shape): uploaded once, then reused with no copy per scan
        swd::DevPtr<swk::DrainArgs> d_drain;
        swd::HostPtr<swk::DrainArgs> h_drain;  // pinned: the copies' sources
        std::vector<std::vector<uint64_t>> drain_keys;  // what each slot's content is a function of
        int drain_next = 0;
        swd::HostPtr<uint64_t> h_trace;  // sw_opts trace_file: host-mapped block timeline
        size_t trace_entries = 0;   // ... its entries: per block, then per merged-launch workgroup
        bool built = false;
        size_t device_bytes = 0;
    };
    Layout lay;
    // the layout's shape (sw_pack.h), assigned by the build that uploaded it:
    // the counts, and of the tables blk_groups, blk_res and llen
    swpack::Shape shape;
    int rid_identity = -1;               // result ids are 0 .. n-1 in order (1), or not (0); -1 unknown
    uint64_t list_epoch = 0;             // fault_epoch() when the lists were last known clean
    // the intra chain's order (adapt_intra_i16_first): the fp16 pass's
    // flagged count (lcount), and per scoring the shortest query seen to flag
    // over a third of the long subjects
    swd::Readback lcount;
    std::vector<std::pair<uint64_t, int32_t>> i16_first;
    // the inter scan's counterpart (adapt_inter_i16_span): the fp16 pass's
    // flagged count and largest flagged block (icount), and per (scoring,
    // query length) the span of widest blocks the int16 kernel then takes first
    swd::Readback icount;
    struct SpanObs {
        uint64_t key;
        int32_t qlen;
        int32_t span;
    };
    std::vector<SpanObs> i16_span;
    int32_t last_ncoop = 0;              // blocks the last scan gave the coop kernel
    int32_t last_npair = 0;              // blocks the last scan ran by wave pairs
    bool last_pair_merged = false;
    // host copies kept to allow re-partitioning when the threshold changes
    std::vector<uint8_t, swd::NoInitAlloc<uint8_t>> h_residues;
    std::vector<int64_t> h_offsets;
    std::vector<int32_t> h_ids;
    std::unordered_map<int32_t, int64_t> id_index;  // result id -> subject (subject_of builds it on first use)
    // subject -> its position in swpack::length_order (position_of builds it
    // on first use: the layout's own order is released after upload); with the
    // layout's nlong, swpack::locate gives where its residues are resident
    std::vector<int64_t> pos_of;
    // synthetic database (sw_db_create_synthetic): residues are generated
    // on the device from (seed, id_base + local id); h_residues stays empty
    bool synthetic = false;
    uint64_t seed = 0;
    int64_t id_base = 0;
};

// A position-specific scoring matrix resident on its handle's device
// (sw_pssm_create): the transposed image swk::PssmProfileArgs describes,
// uploaded once; the host keeps what planning and the adaptive state need.
struct sw_pssm {
    sw_handle* h = nullptr;
    int32_t qlen = 0;
    int32_t ld = 0;               // entries per code row of the image (>= qlen)
    swd::DevPtr<int8_t> d;        // [25][ld]
    std::vector<int8_t> image;    // the upload's source (alive while the copy may run)
    int max_entry = 0;            // the largest entry (0 for an empty table)
    uint64_t hash = 0;            // FNV-1a of the [qlen][25] table
};

namespace swd {

// The C ABI takes a database as const wherever a call computes on it; the
// driver's caches behind it (the layout after a lazy rebuild, the id and
// length tables uploaded on first use, the lookup tables, the adaptive
// observations) are filled by those calls.  The one place that says so.
inline sw_db* mutable_db(const sw_db* db) { return const_cast<sw_db*>(db); }

// Where a scan's (or a traceback's) scores come from: residue codes against
// a 25 x 25 matrix (sc), or a resident position-specific table with its gaps.
// Only build_profiles / scan_profiles (and sw_align's upload) branch on it.
struct QuerySrc {
    const uint8_t* codes = nullptr;
    const sw_scoring* sc = nullptr;
    const sw_pssm* pssm = nullptr;
    int go = 0, ge = 0;  // the PSSM form's gaps
    int32_t qlen = 0;
};
inline QuerySrc seq_src(const uint8_t* q, int32_t qlen, const sw_scoring* sc) {
    return QuerySrc{q, sc, nullptr, 0, 0, qlen};
}
inline QuerySrc pssm_src(const sw_pssm* p, int32_t go, int32_t ge) {
    return QuerySrc{nullptr, nullptr, p, go, ge, p ? p->qlen : 0};
}

// A ranking asked for with a scan (sw_scan_rank_device, sw_scan_topk): the
// k best keys of the scan's scores over the database's subjects — result id
// r, global id gid ? gid[r] : id_base + r — into out (device, k keys).
struct RankReq {
    int32_t k;
    const int32_t* gid;
    int64_t id_base;
    int64_t* out;
};

// ---- sw_scoring.cpp ---------------------------------------------------------
int check_gaps(int go, int ge);
// The matrix (the reference's BLOSUM50 by default) and gaps of sc, validated.
int check_scoring(const sw_scoring* sc, const int8_t** mat, int* go, int* ge);

// ---- sw_handle.cpp ----------------------------------------------------------
// A kernel of this handle reported a fault since the last check: SW_E_DEVICE, once.
int check_fault(sw_handle* h);
// Faults reported so far (any handle): every database re-initialises its
// rescue lists at its first scan after one (sw_db::list_epoch).
uint64_t fault_epoch();
// Wait for everything queued on the handle's streams; the first error.
hipError_t quiesce(sw_handle* h);
// The handle's stream waits for every deferred rescue tail still pending.
int join_tails(sw_handle* h);
// The event set of the next scan becomes h->ev / h->ev_rec.
int next_events(sw_handle* h);

// ---- sw_db.cpp --------------------------------------------------------------
swplan::PlanDb plan_view(const sw_db* db);  // the planning policies' view (sw_plan.h)
int build_db(sw_db* db);                    // pack and upload the layout of db->long_threshold
// Boundary rows of the passes (allocated on first need), and the deferred
// tails' own (false: device memory does not allow them).
int ensure_bnd(sw_db* db, bool affine, bool intra_f);
bool ensure_rbnd(sw_db* db, bool affine, bool intra_f);
// Residues of subject k (host): stored, or regenerated for synthetic dbs.
void subject_residues(const sw_db* db, int64_t k, uint8_t* out);
// The result ids on the device (null: they are 0 .. n-1 in order) and the
// lengths in the same order, each uploaded on first use.
int subject_ids(sw_db* db, const int32_t** rid);
int subject_lengths(sw_db* db, const int32_t** slen);
// The subject with result id `id` (-1: none), and a subject's position in
// swpack::length_order; each owns its table (id_index, pos_of).
int64_t subject_of(sw_db* db, int32_t id);
int64_t position_of(sw_db* db, int64_t subj);

// ---- sw_capi.cpp: the scan driver --------------------------------------------
int check_pssm(const sw_handle* h, const sw_pssm* p, int go, int ge);  // the PSSM entry points' own checks
int check_batch(const int64_t* qoffsets, int32_t nq);  // offsets from 0 up, no query over 2^24
// One scan enqueued on the handle's streams.  defer: another scan follows
// before the caller waits; rq, hist (nullable): rank the scores, build their
// calibration table, before the scan's end event.
int scan_impl(sw_handle* h, const sw_db* db, const QuerySrc& src, int32_t* scores_dev, bool defer = false,
              const RankReq* rq = nullptr, uint32_t* hist = nullptr);
int hist_after(sw_handle* h, sw_db* db, const int32_t* scores_dev, uint32_t* hist_dev);
int ensure_topk_work(sw_handle* h, size_t need);  // the handle's top-K workspace holds `need` bytes

// ---- sw_search.cpp: what sw_refine.cpp builds on -------------------------------
int ensure_scores(sw_handle* h, size_t n);                     // the handle's score buffer holds n int32
int ensure_hist_host(sw_handle* h, size_t n, uint32_t** out);  // its pinned landing area holds n calibration tables
void calib_of(const sw_db* db, const uint32_t* hist, int32_t qlen, sw_calib* out);
// The traceback of ids[0 .. n); msa_dev (nullable, device [n][qlen]): the hits' query-anchored rows too.
int align_impl(sw_handle* h, const sw_db* db, const QuerySrc& src, const int32_t* ids, int32_t n, sw_alignment* out,
               char* ops, int64_t ops_stride, uint8_t* msa_dev);
// The key pass, the selection and (rows_dev non-null) the gather of sw_sig_topk_device, enqueued.
int sig_topk_enqueue(sw_handle* h, sw_db* db, const int32_t* scores_dev, const int32_t* adj_host, int32_t max_len,
                     int64_t r_min, int32_t k, int64_t* keys_out_dev, uint32_t* count_out_dev, int32_t* rows_dev);

}  // namespace swd
