// sw_capi.cpp — host driver behind the C ABI (include/sw_amd.h).
//
// What the reference does per query (SWSolver.cu:266-404) and what replaces it:
//   * pad/encode the query and upload it to __constant__ (:267-299)
//       -> a 32 x qpad int8 query PROFILE (score of every residue code against
//          every query row, pre-biased by the gap for the linear kernels),
//          built on the device by the scan's first launch (sw_profile.hip)
//          from the query's codes (tiny: 32 B/row);
//   * re-pack the whole database into managed memory on every query,
//     longest-first, 32 lanes per block (:301-371)
//       -> sw_db_create packs ONCE into 64-lane blocks of 16-residue groups,
//          sorted longest-first (sw_pack.cpp), and keeps the result resident
//          in HBM;
//   * launch in chunks with cudaDeviceSynchronize after each (:332-354,379)
//       -> one asynchronous launch per kernel on the handle's stream;
//   * read managed scores back in packing order (:383-390)
//       -> kernels write scores[id] directly.
#include <algorithm>
#include <cmath>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "sw_calib.h"
#include "sw_dbfile.h"
#include "sw_host.h"
#include "sw_pack.h"
#include "sw_parallel.h"
#include "sw_plan.h"
#include "sw_synth_host.h"

using swk::DevPtr;
using swk::Event;
using swk::HostPtr;
using swk::parallel_for;
using swk::Stream;

namespace {

thread_local std::string g_err;

// fp16 represents every integer in [-kF16Span, kF16Span] exactly
constexpr int kF16Span = 2048;

// packed fp16 pair (v, v) of a small integer (|v| <= 2048: exact)
uint32_t f16_pair(int v) {
    const _Float16 x = static_cast<_Float16>(static_cast<float>(v));
    uint16_t b;
    std::memcpy(&b, &x, 2);
    return static_cast<uint32_t>(b) | (static_cast<uint32_t>(b) << 16);
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// record event k of the current scan's set on stream s
#define MARK(k, s)                                  \
    do {                                            \
        HIPCHECK(hipEventRecord(h->ev[k].get(), (s)));    \
        *h->ev_rec |= 1u << (k);                    \
    } while (0)

// ---- built-in matrices (code order ARNDCQEGHILKMFPSTWYVBJZX*) ------------
// BLOSUM50 exactly as tabulated in the reference, SWSolver.cu:54-81.
const int8_t kBlosum50Ref[625] = {
    5, -2, -1, -2, -1, -1, -1, 0, -2, -1, -2, -1, -1, -3, -1, 1, 0, -3, -2, 0, -2, -2, -1, -1, 0,
    -2, 7, -1, -2, -4, 1, 0, -3, 0, -4, -3, 3, -2, -3, -3, -1, -1, -3, -1, -3, -1, -3, 0, -1, 0,
    -1, -1, 7, 2, -2, 0, 0, 0, 1, -3, -4, 0, -2, -4, -2, 1, 0, -4, -2, -3, 5, -4, 0, -1, 0,
    -2, -2, 2, 8, -4, 0, 2, -1, -1, -4, -4, -1, -4, -5, -1, 0, -1, -5, -3, -4, 6, -4, 1, -1, 0,
    -1, -4, -2, -4, 13, -3, -3, -3, -3, -2, -2, -3, -2, -2, -4, -1, -1, -5, -3, -1, -3, -2, -3, -1, 0,
    -1, 1, 0, 0, -3, 7, 2, -2, 1, -3, -2, 2, 0, -4, -1, 0, -1, -1, -1, -3, 0, -3, 4, -1, 0,
    -1, 0, 0, 2, -3, 2, 6, -3, 0, -4, -3, 1, -2, -3, -1, -1, -1, -3, -2, -3, 1, -3, 5, -1, 0,
    0, -3, 0, -1, -3, -2, -3, 8, -2, -4, -4, -2, -3, -4, -2, 0, -2, -3, -3, -4, -1, -4, -2, -1, 0,
    -2, 0, 1, -1, -3, 1, 0, -2, 10, -4, -3, 0, -1, -1, -2, -1, -2, -3, 2, -4, 0, -3, 0, -1, 0,
    -1, -4, -3, -4, -2, -3, -4, -4, -4, 5, 2, -3, 2, 0, -3, -3, -1, -3, -1, 4, -4, 4, -3, -1, 0,
    -2, -3, -4, -4, -2, -2, -3, -4, -3, 2, 5, -3, 3, 1, -4, -3, -1, -2, -1, 1, -4, 4, -3, -1, 0,
    -1, 3, 0, -1, -3, 2, 1, -2, 0, -3, -3, 6, -2, -4, -1, 0, -1, -3, -2, -3, 0, -3, 1, -1, 0,
    -1, -2, -2, -4, -2, 0, -2, -3, -1, 2, 3, -2, 7, 0, -3, -2, -1, -1, 0, 1, -3, 2, -1, -1, 0,
    -3, -3, -4, -5, -2, -4, -3, -4, -1, 0, 1, -4, 0, 8, -4, -3, -2, 1, 4, -1, -4, 1, -4, -1, 0,
    -1, -3, -2, -1, -4, -1, -1, -2, -2, -3, -4, -1, -3, -4, 10, -1, -1, -4, -3, -3, -2, -3, -1, -1, 0,
    1, -1, 1, 0, -1, 0, -1, 0, -1, -3, -3, 0, -2, -3, -1, 5, 2, -4, -2, -2, 0, -3, 0, -1, 0,
    0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 2, 5, -3, -2, 0, 0, -1, -1, -1, 0,
    -3, -3, -4, -5, -5, -1, -3, -3, -3, -3, -2, -3, -1, 1, -4, -4, -3, 15, 2, -3, -5, -2, -2, -1, 0,
    -2, -1, -2, -3, -3, -1, -2, -3, 2, -1, -1, -2, 0, 4, -3, -2, -2, 2, 8, -1, -3, -1, -2, -1, 0,
    0, -3, -3, -4, -1, -3, -3, -4, -4, 4, 1, -3, 1, -1, -3, -2, 0, -3, -1, 5, -3, 2, -3, -1, 0,
    -2, -1, 5, 6, -3, 0, 1, -1, 0, -4, -4, 0, -3, -4, -2, 0, 0, -5, -3, -3, 6, -4, 1, -1, 0,
    -2, -3, -4, -4, -2, -3, -3, -4, -3, 4, 4, -3, 2, 1, -3, -3, -1, -2, -1, 2, -4, 4, -3, -1, 0,
    -1, 0, 0, 1, -3, 4, 5, -2, 0, -3, -3, 1, -1, -4, -1, 0, -1, -2, -2, -3, 1, -3, 5, -1, 0,
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
};

// NCBI BLOSUM62 with J; an option of this build (the reference has none).
const int8_t kBlosum62[625] = {
    4, -1, -2, -2, 0, -1, -1, 0, -2, -1, -1, -1, -1, -2, -1, 1, 0, -3, -2, 0, -2, -1, -1, 0, -4,
    -1, 5, 0, -2, -3, 1, 0, -2, 0, -3, -2, 2, -1, -3, -2, -1, -1, -3, -2, -3, -1, -2, 0, -1, -4,
    -2, 0, 6, 1, -3, 0, 0, 0, 1, -3, -3, 0, -2, -3, -2, 1, 0, -4, -2, -3, 3, -3, 0, -1, -4,
    -2, -2, 1, 6, -3, 0, 2, -1, -1, -3, -4, -1, -3, -3, -1, 0, -1, -4, -3, -3, 4, -3, 1, -1, -4,
    0, -3, -3, -3, 9, -3, -4, -3, -3, -1, -1, -3, -1, -2, -3, -1, -1, -2, -2, -1, -3, -1, -3, -2, -4,
    -1, 1, 0, 0, -3, 5, 2, -2, 0, -3, -2, 1, 0, -3, -1, 0, -1, -2, -1, -2, 0, -2, 3, -1, -4,
    -1, 0, 0, 2, -4, 2, 5, -2, 0, -3, -3, 1, -2, -3, -1, 0, -1, -3, -2, -2, 1, -3, 4, -1, -4,
    0, -2, 0, -1, -3, -2, -2, 6, -2, -4, -4, -2, -3, -3, -2, 0, -2, -2, -3, -3, -1, -4, -2, -1, -4,
    -2, 0, 1, -1, -3, 0, 0, -2, 8, -3, -3, -1, -2, -1, -2, -1, -2, -2, 2, -3, 0, -3, 0, -1, -4,
    -1, -3, -3, -3, -1, -3, -3, -4, -3, 4, 2, -3, 1, 0, -3, -2, -1, -3, -1, 3, -3, 3, -3, -1, -4,
    -1, -2, -3, -4, -1, -2, -3, -4, -3, 2, 4, -2, 2, 0, -3, -2, -1, -2, -1, 1, -4, 3, -3, -1, -4,
    -1, 2, 0, -1, -3, 1, 1, -2, -1, -3, -2, 5, -1, -3, -1, 0, -1, -3, -2, -2, 0, -3, 1, -1, -4,
    -1, -1, -2, -3, -1, 0, -2, -3, -2, 1, 2, -1, 5, 0, -2, -1, -1, -1, -1, 1, -3, 2, -1, -1, -4,
    -2, -3, -3, -3, -2, -3, -3, -3, -1, 0, 0, -3, 0, 6, -4, -2, -2, 1, 3, -1, -3, 0, -3, -1, -4,
    -1, -2, -2, -1, -3, -1, -1, -2, -2, -3, -3, -1, -2, -4, 7, -1, -1, -4, -3, -2, -2, -3, -1, -2, -4,
    1, -1, 1, 0, -1, 0, 0, 0, -1, -2, -2, 0, -1, -2, -1, 4, 1, -3, -2, -2, 0, -2, 0, 0, -4,
    0, -1, 0, -1, -1, -1, -1, -2, -2, -1, -1, -1, -1, -2, -1, 1, 5, -2, -2, 0, -1, -1, -1, 0, -4,
    -3, -3, -4, -4, -2, -2, -3, -2, -2, -3, -2, -3, -1, 1, -4, -3, -2, 11, 2, -3, -4, -2, -3, -2, -4,
    -2, -2, -2, -3, -2, -1, -2, -3, 2, -1, -1, -2, -1, 3, -3, -2, -2, 2, 7, -1, -3, -1, -2, -1, -4,
    0, -3, -3, -3, -1, -2, -2, -3, -3, 3, 1, -2, 1, -1, -2, -2, 0, -3, -1, 4, -3, 2, -2, -1, -4,
    -2, -1, 3, 4, -3, 0, 1, -1, 0, -3, -4, 0, -3, -3, -2, 0, -1, -4, -3, -3, 4, -3, 1, -1, -4,
    -1, -2, -3, -3, -1, -2, -3, -4, -3, 3, 3, -3, 2, 0, -3, -2, -1, -2, -1, 2, -3, 3, -3, -1, -4,
    -1, 0, 0, 1, -3, 3, 4, -2, 0, -3, -3, 1, -1, -3, -1, 0, -1, -3, -2, -2, 1, -3, 4, -1, -4,
    0, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, 0, 0, -2, -1, -1, -1, -1, -1, -1, -4,
    -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, 1,
};

int8_t g_encode_lut[256];
bool g_lut_ready = false;

void init_lut() {
    if (g_lut_ready) return;
    static const char letters[] = "ARNDCQEGHILKMFPSTWYVBJZX";  // SWSolver.cu:17-40
    for (int c = 0; c < 256; ++c) g_encode_lut[c] = SW_CODE_STAR;  // SWSolver.cu:119
    for (int k = 0; k < 24; ++k) g_encode_lut[static_cast<unsigned char>(letters[k])] = static_cast<int8_t>(k);
    g_lut_ready = true;
}

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

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

}  // namespace

int swk::set_error(int code, const std::string& msg) { return fail(code, msg); }

// ---------------------------------------------------------------------------
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

namespace {
sw_opts default_opts() {
    sw_opts o;
    std::memset(&o, 0, sizeof o);
    o.size = static_cast<int32_t>(sizeof o);
    for (int32_t* f : {&o.lpt, &o.lpt_pipe, &o.quad_width, &o.pair_width, &o.pair_group, &o.coop_width,
                       &o.coop_skew, &o.intra_x2, &o.intra_x2_rows, &o.intra_i16_first, &o.inter_i16_span,
                       &o.int16_guard, &o.rescue_stats, &o.tail_pairs, &o.lpt_persist, &o.lpt_rows,
                       &o.tri_width, &o.lpt_pipe_tail, &o.drain_spin})
        *f = -1;
    return o;
}
}  // namespace

struct sw_handle {
    int device = 0;
    int cus = 0;  // compute units of the device
    Stream stream;  // the handle's own, or the caller's (sw_set_stream): borrowed, given up
    bool own_stream = false;  // ... before the owner would destroy it
    ~sw_handle() { if (!own_stream) stream.release(); }
    // One event set per scan since the last sw_timing_reset (grows as needed,
    // reused after a reset), so a caller can time many back-to-back scans
    // without synchronising between them.
    std::vector<ScanEvents> evpool;
    size_t nscans = 0;
    Event* ev = nullptr;  // event set of the current scan (an alias into evpool, as ev_rec)
    unsigned* ev_rec = nullptr;
    // The intra kernel runs on a side stream, concurrently with the inter
    // kernel (fork/join through ev[0] and ev[1]).
    Stream side;
    Stream side2;  // the cooperative wide-block kernel
    // Deferred rescue tails (the queries of a batch but the last): a scan's
    // re-scoring stages (int16 / int32 list kernels) run on `tail` after its
    // fp16 passes, while the next query's fp16 passes start on the main and
    // side streams.  Lists and boundary rows of the tail are its own
    // (parity-indexed lists, sw_db::d_rbnd_*), so nothing is shared with the
    // passes running beside it.
    Stream tail;
    Event main_done, side_done;  // fp16 passes of the scan being deferred
    Event tail_done[2];  // per list parity
    bool tail_pending[2] = {};
    int parity = 0;                                       // list set of the next scan
    Event coop_done;
    Event fork2;  // side2 starts after the rescue counters are reset
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
        DevPtr<int8_t> d;
        size_t dcap = 0;
        // the end event (ev[3]) of the slot's last scan: reusing the slot
        // waits for it.  Not an event of its own: each event record is a
        // packet the command processor spends ~5 us on between two kernels
        // (rocprofv3 trace of C2's 1/8 share, scripts/step_gaps.py)
        hipEvent_t last_end = nullptr;  // (an alias into evpool)
        bool pending = false;
        Event tail_read;  // a deferred rescue tail has read the slot
        bool tail_pending = false;
    };
    // pinned staging of database uploads (build_db): the host packs one
    // buffer while the other's copy runs
    HostPtr<uint8_t> stage[2];
    size_t stage_cap = 0;
    Event stage_ev[2];
    bool stage_pending[2] = {};
    static constexpr int kProfSlots = 4;
    ProfSlot prof[kProfSlots];
    int prof_next = 0;
    DevPtr<int32_t> d_scores;  // for the synchronous sw_scan
    size_t scores_cap = 0;
    DevPtr<int64_t> d_topk_work;  // device top-K workspace
    DevPtr<uint32_t> d_hist;      // the calibration table of the synchronous sw_score_hist
    // pinned landing area of the scans' calibration tables (the _sig and _calib
    // forms): a copy into pageable memory would make the host wait inside
    // hipMemcpyAsync, one more synchronisation in all but name
    HostPtr<uint32_t> h_hist;
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
    HostPtr<int32_t> h_fault;
    int32_t* d_fault = nullptr;  // the device address of h_fault (an alias)
    int open_slot = -1;  // profile slot pending on an ev[3] this scan has not recorded yet
    sw_opts opts = default_opts();  // kernel-form overrides (sw_set_opts); all -1 = the library's choice
};

// Faults reported so far (any handle): a drain that gave up on an entry
// left claimed entries of its database's rescue lists un-reset, so every
// database re-initialises its lists at its first scan after a fault
// (sw_db::list_epoch) and later scans are exact again.
static std::atomic<uint64_t> g_fault_epoch{0};

// A kernel of this handle reported a fault since the last check (sw_kernels.h
// list_wait_take): fail loudly, once.
static int check_fault(sw_handle* h) {
    if (h && h->h_fault.get() && __atomic_load_n(h->h_fault.get(), __ATOMIC_ACQUIRE)) {
        __atomic_store_n(h->h_fault.get(), 0, __ATOMIC_RELEASE);
        g_fault_epoch.fetch_add(1);
        return fail(SW_E_DEVICE, "sw_scan_lpt: a claimed rescue-list entry never appeared; the handle's scans "
                                 "since the last successful call may hold unrescued scores");
    }
    return SW_OK;
}

// Wait for everything queued on the handle's streams (before a release, or
// after a failed scan); the first error, for the callers that check.
static hipError_t quiesce(sw_handle* h) {
    hipError_t first = hipSuccess;
    for (hipStream_t st : {h->stream.get(), h->side.get(), h->side2.get(), h->tail.get()})
        if (st) {
            const hipError_t e = hipStreamSynchronize(st);
            if (first == hipSuccess) first = e;
        }
    return first;
}

// What a scan's fp16 pass flagged, read back without waiting: one or two
// device words copied to a pinned pair in stream order behind the pass, an
// event after the copy, and what the readback observes.  A later scan takes
// it once the event has completed (the adaptive routes, adapt_*); a scan
// repeating the last observation taken does not read it back again.
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
};

namespace {
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

// Forget the pending and the last observation.  A readback still in flight
// lands in the same pinned words later, in stream order before any readback
// a later scan issues: ignoring it is safe.
void readback_reset(Readback& r) { r.pending = r.seen = false; }

}  // namespace

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
        DevPtr<int32_t> d_order;
        std::vector<float> cost;  // estimated duration of each entry, longest first
    };
    static constexpr int kDrainSlots = 32;
    // Everything that belongs to one packed layout (one long threshold):
    // build_db and the scans after it fill it, free_dev replaces it with a
    // fresh one.  What a member of sw_db outside it holds survives a rebuild.
    struct Layout {
        // inter part
        DevPtr<uint8_t> d_res;
        DevPtr<uint64_t> d_blk_off;
        DevPtr<uint32_t> d_blk_groups;
        DevPtr<uint32_t> d_blk_cols;  // block widths rounded to 8 columns (sw_inter_x2s)
        DevPtr<int32_t> d_lane_ids;
        DevPtr<int32_t> d_ids;        // every subject's result id (sw_scan_topk), on first use
        DevPtr<int32_t> d_slen;       // every subject's length, in the same order (sw_score_hist), on first use
        DevPtr<int32_t> d_bnd_h, d_bnd_f;
        // two rescue lists [count, block ids...] of nblocks + 1 ints each: the
        // 16-bit kernels' flagged blocks (list A), and the fp16 chain's second
        // stage's (list B)
        // (two parities of these lists: consecutive scans of a batch alternate)
        DevPtr<int32_t> d_rescue;
        DevPtr<int32_t> d_lrescue;    // [count, subjects...] x 2: the intra rescue chain's lists
        // boundary rows of deferred rescue tails (inter H, F; intra H, F), when
        // device memory allows them (else the tails run in stream order)
        DevPtr<int32_t> d_rbnd_h, d_rbnd_f, d_rlbnd_h, d_rlbnd_f;
        bool rbnd_tried = false;
        // intra part (long subjects)
        DevPtr<uint8_t> d_lres;
        DevPtr<uint64_t> d_loff;
        DevPtr<int32_t> d_llen, d_lid, d_lbnd_h, d_lbnd_f;
        std::vector<LptTable> lpt_tables;
        // device copies of the merged launch's drain arguments (swk::DrainArgs),
        // one per distinct content (profile slot x list parity x score buffer
        // x query shape): uploaded once, then reused with no copy per scan
        DevPtr<swk::DrainArgs> d_drain;
        HostPtr<swk::DrainArgs> h_drain;  // pinned: the copies' sources
        std::vector<std::vector<uint64_t>> drain_keys;  // what each slot's content is a function of
        int drain_next = 0;
        HostPtr<uint64_t> h_trace;  // sw_opts trace_file: host-mapped block timeline
        size_t trace_entries = 0;   // ... its entries: per block, then per merged-launch workgroup
        bool built = false;
        size_t device_bytes = 0;
    };
    Layout lay;
    // the layout's shape (sw_pack.h), assigned by the build that uploaded it:
    // the counts, and of the tables blk_groups, blk_res and llen
    swpack::Shape shape;
    int rid_identity = -1;               // result ids are 0 .. n-1 in order (1), or not (0); -1 unknown
    uint64_t list_epoch = 0;             // g_fault_epoch when the lists were last known clean
    // the intra chain's order (adapt_intra_i16_first): the fp16 pass's
    // flagged count (lcount), and per scoring the shortest query seen to flag
    // over a third of the long subjects
    Readback lcount;
    std::vector<std::pair<uint64_t, int32_t>> i16_first;
    // the inter scan's counterpart (adapt_inter_i16_span): the fp16 pass's
    // flagged count and largest flagged block (icount), and per (scoring,
    // query length) the span of widest blocks the int16 kernel then takes first
    Readback icount;
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
    std::vector<uint8_t, NoInitAlloc<uint8_t>> h_residues;
    std::vector<int64_t> h_offsets;
    std::vector<int32_t> h_ids;
    std::unordered_map<int32_t, int64_t> id_index;  // result id -> subject (built on first sw_align)
    // subject -> its position in swpack::length_order (built on first
    // sw_hit_stats: the layout's own order is released after upload); with the
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
    DevPtr<int8_t> d;             // [25][ld]
    std::vector<int8_t> image;    // the upload's source (alive while the copy may run)
    int max_entry = 0;            // the largest entry (0 for an empty table)
    uint64_t hash = 0;            // FNV-1a of the [qlen][25] table
};

namespace {

// The planning policies' view of a database (sw_plan.h).
swplan::PlanDb plan_view(const sw_db* db) {
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

// sw_db_reset_adaptive: forget what earlier scans observed.
void reset_adaptive(sw_db* db) {
    readback_reset(db->lcount);
    db->i16_first.clear();
    readback_reset(db->icount);
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

// Residues of subject k (host): stored, or regenerated for synthetic dbs.
void subject_residues(const sw_db* db, int64_t k, uint8_t* out) {
    const int64_t L = db->h_offsets[k + 1] - db->h_offsets[k];
    if (db->synthetic)
        swk::synth_residues(db->seed, static_cast<uint64_t>(db->id_base + db->h_ids[k]), L, out);
    else
        std::memcpy(out, db->h_residues.data() + db->h_offsets[k], L);
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

// The device half of packing: the layout's shape is sw_pack.cpp's; allocate
// it, upload the residues as the packer fills them (or generate them in
// place), upload its tables, and keep the shape.
int build_db(sw_db* db) {
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
int ensure_bnd(sw_db* db, bool affine, bool intra_f) {
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
bool ensure_rbnd(sw_db* db, bool affine, bool intra_f) {
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

int check_gaps(int go, int ge) {
    if (go <= 0 || ge <= 0 || go > 1000 || ge > 1000) return fail(SW_E_INVALID, "gap penalties must be in 1..1000");
    return SW_OK;
}

int check_scoring(const sw_scoring* sc, const int8_t** mat, int* go, int* ge) {
    *mat = kBlosum50Ref;
    *go = 2;
    *ge = 2;
    if (sc) {
        if (sc->matrix) *mat = sc->matrix;
        *go = sc->gap_open;
        *ge = sc->gap_extend;
    }
    if (int rc = check_gaps(*go, *ge)) return rc;
    for (int k = 0; k < 625; ++k)
        if ((*mat)[k] < -100 || (*mat)[k] > 100) return fail(SW_E_INVALID, "matrix entries must be in -100..100");
    return SW_OK;
}

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
QuerySrc seq_src(const uint8_t* q, int32_t qlen, const sw_scoring* sc) {
    QuerySrc s;
    s.codes = q;
    s.qlen = qlen;
    s.sc = sc;
    return s;
}
QuerySrc pssm_src(const sw_pssm* p, int32_t go, int32_t ge) {
    QuerySrc s;
    s.pssm = p;
    s.qlen = p ? p->qlen : 0;
    s.go = go;
    s.ge = ge;
    return s;
}
// The PSSM entry points' own argument checks (the handle and the database are
// the shared paths').
int check_pssm(const sw_handle* h, const sw_pssm* p, int go, int ge) {
    if (!h || !p) return fail(SW_E_INVALID, "null argument");
    if (p->h->device != h->device) return fail(SW_E_INVALID, "the PSSM was created on another handle's device");
    return check_gaps(go, ge);
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
    const int bias = affine ? 0 : go;
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
    const int rip = swk::intra_rip(ri);
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
    if (src.pssm) {
        swk::PssmProfileArgs a{};
        a.p8 = S.d.get() + P->off8;
        a.p16 = want16 ? reinterpret_cast<int16_t*>(S.d.get() + P->off16) : nullptr;
        a.pin = ri ? S.d.get() + P->intra_off : nullptr;
        a.stride = P->stride;
        a.qlen = qlen;
        a.bias = bias;
        a.ri = ri;
        a.rip = rip;
        a.qpad_intra = ri ? qpad_intra : 0;
        a.rows = std::max(P->stride, a.qpad_intra);
        for (int k = 0; k < 10; ++k) a.reset[k] = reset[k];
        a.pssm = src.pssm->d.get();
        a.ld = src.pssm->ld;
        HIPCHECK(swk::launch_build_profile_pssm(a, h->stream.get()));
        S.last_end = h->ev[3].get();
        S.pending = true;
        h->open_slot = P->slot;
        return SW_OK;
    }
    swk::ProfileArgs a{};
    a.p8 = S.d.get() + P->off8;
    a.p16 = want16 ? reinterpret_cast<int16_t*>(S.d.get() + P->off16) : nullptr;
    a.pin = ri ? S.d.get() + P->intra_off : nullptr;
    a.stride = P->stride;
    a.qlen = qlen;
    a.bias = bias;
    a.ri = ri;
    a.rip = rip;
    a.qpad_intra = ri ? qpad_intra : 0;
    for (int k = 0; k < 10; ++k) a.reset[k] = reset[k];
    std::memcpy(a.mat, mat, 625);
    const int32_t rows = std::max(P->stride, a.qpad_intra);
    for (int32_t r0 = 0; r0 < rows; r0 += swk::kProfQueryChunk) {
        a.row0 = r0;
        a.row1 = std::min(rows, r0 + swk::kProfQueryChunk);
        const int32_t nq = std::max(0, std::min(a.row1, qlen) - r0);
        if (nq) std::memcpy(a.q, q + r0, static_cast<size_t>(nq));
        HIPCHECK(swk::launch_build_profile(a, h->stream.get()));
        for (auto& p : a.reset) p = nullptr;  // once
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

// The handle's stream waits for every deferred rescue tail still pending, so
// what completes on it (a non-deferred scan, the end of a batch) includes
// the rescued scores of the scans before it.
int join_tails(sw_handle* h) {
    for (int q = 0; q < 2; ++q)
        if (h->tail_pending[q]) {
            HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->tail_done[q].get(), 0));
            h->tail_pending[q] = false;
        }
    return SW_OK;
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

// A database's result ids on the device (db->lay.d_ids, uploaded on first
// use), or null when the ids are 0 .. n-1 in order (the default).
int subject_ids(sw_db* db, const int32_t** rid) {
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

// The ranking input over a database's subjects: its scores through the
// result ids, or directly when those are the identity.
int rank_src(sw_db* db, const int32_t* scores, const RankReq& rq, swk::TopkSrc* src) {
    *src = swk::TopkSrc{};
    src->scores = scores;
    src->gid = rq.gid;
    src->id_base = rq.id_base;
    return subject_ids(db, &src->rid);
}

// The calibration table of a score array over a database's subjects
// (sw_calib.hip): the table zeroed, then one count per subject, on the
// handle's stream.  The subjects' lengths go up on first use, in the
// database's own order (beside d_ids: whatever the long threshold is, the
// table is the same).
int hist_after(sw_handle* h, sw_db* db, const int32_t* scores_dev, uint32_t* hist_dev) {
    HIPCHECK(hipMemsetAsync(hist_dev, 0, swcalib::kCells * sizeof(uint32_t), h->stream.get()));
    if (db->n == 0) return SW_OK;
    const int32_t* rid = nullptr;
    if (int rc = subject_ids(db, &rid)) return rc;
    if (!db->lay.d_slen.get()) {
        std::vector<int32_t> L(static_cast<size_t>(db->n));
        for (int64_t k = 0; k < db->n; ++k) L[k] = static_cast<int32_t>(db->h_offsets[k + 1] - db->h_offsets[k]);
        HIPCHECK(swk::dev_alloc(db->lay.d_slen, L.size() * sizeof(int32_t)));
        HIPCHECK(hipMemcpy(db->lay.d_slen.get(), L.data(), L.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        db->lay.device_bytes += L.size() * sizeof(int32_t);
    }
    HIPCHECK(swk::launch_score_hist(scores_dev, rid, db->lay.d_slen.get(), db->n, hist_dev, h->stream.get()));
    ++h->launches;
    return SW_OK;
}

// The handle's top-K workspace holds at least `need` bytes; a new one
// starts with the one-launch top-K's counter at zero (swk::launch_topk).
int ensure_topk_work(sw_handle* h, size_t need) {
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

int next_events(sw_handle* h) {
    if (h->nscans >= 4096) h->nscans = 0;  // bound the pool; older sums are dropped
    if (h->nscans == h->evpool.size()) {
        ScanEvents se;
        for (auto& e : se.ev) HIPCHECK(swk::event_create(e));
        h->evpool.push_back(std::move(se));
    }
    h->ev = h->evpool[h->nscans].ev;
    h->ev_rec = &h->evpool[h->nscans].rec;
    *h->ev_rec = 0;
    h->evpool[h->nscans].launches = 0;
    h->evpool[h->nscans].merged = false;
    ++h->nscans;
    return SW_OK;
}

// A scan's ranking: a top-K launch on the scan's stream after every stage
// that writes its scores.
int rank_after(sw_handle* h, sw_db* db, const int32_t* scores_dev, const RankReq& rq) {
    swk::TopkSrc src;
    int rc;
    if ((rc = rank_src(db, scores_dev, rq, &src))) return rc;
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
    MARK(0, h->stream.get());
    if (db->max_id >= 0) HIPCHECK(hipMemsetAsync(scores_dev, 0, static_cast<size_t>(db->max_id + 1) * 4, h->stream.get()));
    if (rq && (rc = rank_after(h, db, scores_dev, *rq))) return rc;
    if (hist && (rc = hist_after(h, db, scores_dev, hist))) return rc;
    for (int k = 1; k < 8; ++k) MARK(k, h->stream.get());
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
    if (db->list_epoch != g_fault_epoch.load()) {  // a fault since: entries may be left claimed
        if ((rc = join_tails(h))) return rc;
        hipStream_t const s = h->stream.get();
        if (int32_t* l = db->lay.d_rescue.get()) HIPCHECK(hipMemsetAsync(l, 0xff, 2 * rstride * sizeof(int32_t), s));
        if (int32_t* l = db->lay.d_lrescue.get()) HIPCHECK(hipMemsetAsync(l, 0xff, 2 * lstride * sizeof(int32_t), s));
        db->list_epoch = g_fault_epoch.load();
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
        MARK(4, h->side2.get());
        HIPCHECK(swk::launch_inter_coop(k, p.ncoop, p.affine, h->opts.coop_skew != 0, h->side2.get()));
        MARK(5, h->side2.get());
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
        MARK(4, h->side2.get());
        HIPCHECK(swk::launch_inter_x2p(k, p.affine, false, false, 2, h->side2.get()));
        MARK(5, h->side2.get());
        HIPCHECK(hipEventRecord(h->coop_done.get(), h->side2.get()));
        ++h->launches;
    }
    MARK(6, h->stream.get());
    if (p.npair)  // one launch: pairs for blocks [nr, npair), one wave per block after
        HIPCHECK(swk::launch_inter_x2p(c.a, p.affine, p.f16, true, swplan::pair_group(plan_view(c.db)), h->stream.get()));
    else
        HIPCHECK(swk::launch_inter(c.a, p.affine, p.shape, h->stream.get()));
    MARK(7, h->stream.get());
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
    MARK(6, h->stream.get());
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
    if (!p.drain) MARK(7, h->stream.get());
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

// defer: another scan follows on this handle before the caller waits (the
// queries of a batch but the last): this scan's rescue tail may run on the
// tail stream beside the next scan's fp16 passes (sw_handle::tail).
// rq (nullable): rank the scan's scores too (a top-K launch after every
// stage that writes them, before the scan's end event).
// hist (nullable, device): the scores' calibration table too (hist_after), at
// the same place: after every stage that writes them, before the end event.
// src: the query source.  The two forms differ in the scoring's checks and
// keys here and in scan_profiles; everything else is one path.
int scan_impl_body(sw_handle* h, const sw_db* cdb, const QuerySrc& src, int32_t* scores_dev, bool defer = false,
                   const RankReq* rq = nullptr, uint32_t* hist = nullptr) {
    sw_db* db = const_cast<sw_db*>(cdb);
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
        MARK(0, h->stream.get());
        if (db->shape.nlong && (rc = long_pass(c))) return rc;
        MARK(1, db->shape.nlong ? h->side.get() : h->stream.get());
        if (db->shape.nblocks && (rc = inter_pass(c))) return rc;
    }
    if ((rc = deferred_tails(c))) return rc;

    // join (the merged launch has no separate inter end, nor a side stream
    // to join), rank, and the end event
    if (!db->shape.nblocks)
        for (int k = 6; k < 8; ++k) MARK(k, h->stream.get());
    if (!p.lpt) MARK(2, h->stream.get());
    if (db->shape.nlong && !p.lpt) HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->ev[1].get(), 0));
    // the scan completes on the handle's stream: so do earlier deferred tails
    if (!c.deferred && (rc = join_tails(h))) return rc;
    if (rq && (rc = rank_after(h, db, scores_dev, *rq))) return rc;
    if (hist && (rc = hist_after(h, db, scores_dev, hist))) return rc;
    MARK(3, h->stream.get());
    h->open_slot = -1;
    h->evpool[h->nscans - 1].launches = h->launches;
    h->timed = true;
    return h->opts.rescue_stats == 1 ? print_rescue_stats(c) : SW_OK;
}

// A scan that fails after its profiles were built leaves the profile slot
// pending on an end event it never recorded: a later scan reusing the slot
// would not wait for the kernels this one queued.  Drain the handle's streams
// and release the slot instead.
int scan_impl(sw_handle* h, const sw_db* db, const QuerySrc& src, int32_t* scores_dev, bool defer = false,
              const RankReq* rq = nullptr, uint32_t* hist = nullptr) {
    const int rc = scan_impl_body(h, db, src, scores_dev, defer, rq, hist);
    if (h && h->open_slot >= 0) {
        (void)quiesce(h);
        h->prof[h->open_slot].pending = false;
        h->open_slot = -1;
    }
    return rc;
}

int scan_impl(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
              int32_t* scores_dev, bool defer = false, const RankReq* rq = nullptr, uint32_t* hist = nullptr) {
    return scan_impl(h, db, seq_src(query, qlen, sc), scores_dev, defer, rq, hist);
}

int ensure_scores(sw_handle* h, size_t n) {
    if (n > h->scores_cap) {
        h->scores_cap = 0;
        const size_t cap = std::max<size_t>(n, 1024);
        HIPCHECK(swk::dev_alloc(h->d_scores, cap * 4));  // the old one released first: ~1 GiB (sw_scan_batch)
        h->scores_cap = cap;
    }
    return SW_OK;
}

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

// sw_scan_topk / sw_scan_pssm_topk: a scan and its ranking, k keys copied back.
// hist_host (nullable): the scan's calibration table too (sw_calib.h), built
// behind the keys in device memory and copied back with them.
int scan_topk_host(sw_handle* h, const sw_db* cdb, const QuerySrc& src, int32_t k, int64_t* keys_host,
                   uint32_t* hist_host = nullptr) {
    sw_db* db = const_cast<sw_db*>(cdb);
    if (!h || !db || !keys_host || k <= 0 || k > 4096) return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (db->n == 0) {
        for (int32_t i = 0; i < k; ++i) keys_host[i] = INT64_MIN;
        if (hist_host) std::memset(hist_host, 0, swcalib::kCells * sizeof(uint32_t));
        return SW_OK;
    }
    int rc;
    HIPCHECK(hipSetDevice(h->device));
    const size_t slots = static_cast<size_t>(db->max_id + 1);
    // scores, then the k keys, then the table
    if ((rc = ensure_scores(h, slots + static_cast<size_t>(2 * k) + 2 + (hist_host ? swcalib::kCells : 0)))) return rc;
    int64_t* keys_dev = reinterpret_cast<int64_t*>(h->d_scores.get() + round_up(static_cast<int64_t>(slots), 2));
    uint32_t* hist_dev = hist_host ? reinterpret_cast<uint32_t*>(keys_dev + k) : nullptr;
    // the ranking runs over the result ids of the subjects (rank_src)
    const RankReq rq{k, nullptr, 0, keys_dev};
    if ((rc = scan_impl(h, db, src, h->d_scores.get(), false, &rq, hist_dev))) return rc;
    HIPCHECK(hipMemcpyAsync(keys_host, keys_dev, static_cast<size_t>(k) * sizeof(int64_t), hipMemcpyDeviceToHost,
                            h->stream.get()));
    if (hist_host)
        HIPCHECK(hipMemcpyAsync(hist_host, hist_dev, swcalib::kCells * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    return check_fault(h);
}

}  // namespace

namespace {
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

// ===========================================================================
extern "C" {

// 0.2: sw_pssm_*; 0.3: sw_hit_stats, sw_scan_hits; 0.4: sw_scan_batch_topk, sw_*_hits batch forms;
// 0.5: sw_score_hist*, sw_calib_*, the _sig and _calib scan forms
int32_t sw_version(void) { return 10000 * 0 + 100 * 5 + 0; }

#ifndef SW_SOURCE_ID
#define SW_SOURCE_ID "unknown"
#endif
const char* sw_build_id(void) { return SW_SOURCE_ID; }

const char* sw_last_error(void) { return g_err.c_str(); }

int sw_encode(const char* ascii, int64_t n, uint8_t* codes) {
    if ((!ascii || !codes) && n > 0) return fail(SW_E_INVALID, "null argument");
    init_lut();
    for (int64_t i = 0; i < n; ++i) codes[i] = static_cast<uint8_t>(g_encode_lut[static_cast<unsigned char>(ascii[i])]);
    return SW_OK;
}

int sw_builtin_matrix(int32_t id, int8_t* out625) {
    if (!out625) return fail(SW_E_INVALID, "null argument");
    if (id == SW_MATRIX_BLOSUM50_REF) {
        std::memcpy(out625, kBlosum50Ref, 625);
    } else if (id == SW_MATRIX_BLOSUM62) {
        std::memcpy(out625, kBlosum62, 625);
    } else if (id == SW_MATRIX_IDENTITY3) {
        for (int a = 0; a < 25; ++a)
            for (int b = 0; b < 25; ++b) out625[a * 25 + b] = static_cast<int8_t>(a == b ? 3 : -3);
    } else if (id == SW_MATRIX_BLOSUM50_CHAR) {
        // the letters score as BLOSUM50_REF; '*' (and
        // everything convertStringToChar maps to it) -5, '*' vs '*' +1
        std::memcpy(out625, kBlosum50Ref, 625);
        for (int k = 0; k < 25; ++k) out625[SW_CODE_STAR * 25 + k] = out625[k * 25 + SW_CODE_STAR] = -5;
        out625[SW_CODE_STAR * 25 + SW_CODE_STAR] = 1;
    } else {
        return fail(SW_E_INVALID, "unknown matrix id");
    }
    return SW_OK;
}

int sw_create(int32_t device, sw_handle** out) {
    if (!out) return fail(SW_E_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SW_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(SW_E_INVALID, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    std::unique_ptr<sw_handle> h(new (std::nothrow) sw_handle());
    if (!h) return fail(SW_E_NOMEM, "out of host memory");
    h->device = device;
    // the device's CUs, once (the merged launch's slot counts: lpt_tail_blocks,
    // the looped grid's size)
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) h->cus = 0;
    HIPCHECK(swk::stream_create(h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    // side and side2 are created with the handle, right after its own
    // stream: HIP maps normal-priority streams onto GPU_MAX_HW_QUEUES (4)
    // hardware queues, least-used first, and two streams sharing a queue run
    // in order.  Created here they take the queues beside the own stream.
    // Created on first use instead, side2 shared the caller's queue
    // and the int16 launch beside the fp16 one ran after it (C3 under the
    // reference scoring 12,840 -> 8,900 GCUPS).
    HIPCHECK(swk::stream_create(h->side, hipStreamNonBlocking));
    HIPCHECK(swk::stream_create(h->side2, hipStreamNonBlocking));
    // The deferred rescue tails (batches) run at high priority: HIP serves
    // those streams from a separate queue pool, so a tail never shares a
    // hardware queue with the next query's scan (sharing one, the next
    // scan waited behind the tail: C3, the reference scoring's long queries
    // stalled 9-13 ms each behind their int16 list kernel).
    int least = 0, greatest = 0;
    HIPCHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHECK(swk::stream_create(h->tail, hipStreamNonBlocking, greatest));
    for (Event* ev : {&h->main_done, &h->side_done, &h->tail_done[0], &h->tail_done[1], &h->coop_done, &h->fork2,
                      &h->stage_ev[0], &h->stage_ev[1]})
        HIPCHECK(swk::event_create(*ev, hipEventDisableTiming));
    for (auto& S : h->prof) HIPCHECK(swk::event_create(S.tail_read, hipEventDisableTiming));
    HIPCHECK(swk::host_alloc(h->h_fault, sizeof(int32_t), hipHostMallocMapped));
    *h->h_fault.get() = 0;
    HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_fault), h->h_fault.get(), 0));
    *out = h.release();
    return SW_OK;
}

int sw_destroy(sw_handle* h) {
    if (!h) return SW_OK;
    (void)hipSetDevice(h->device);
    (void)quiesce(h);
    delete h;
    return SW_OK;
}

void* sw_stream(sw_handle* h) { return h ? reinterpret_cast<void*>(h->stream.get()) : nullptr; }

int sw_opts_init(sw_opts* o) {
    if (!o) return fail(SW_E_INVALID, "null argument");
    *o = default_opts();
    return SW_OK;
}

// The one place the library reads its SW_* variables (tests and A/B scripts
// call it; the scan path reads the handle's sw_opts only).
int sw_opts_from_env(sw_opts* o) {
    int rc;
    if ((rc = sw_opts_init(o))) return rc;
    const struct {
        const char* name;
        int32_t* field;
    } ints[] = {{"SW_LPT", &o->lpt},
                {"SW_LPT_PIPE", &o->lpt_pipe},
                {"SW_QUAD_WIDTH", &o->quad_width},
                {"SW_PAIR_WIDTH", &o->pair_width},
                {"SW_PAIR_GROUP", &o->pair_group},
                {"SW_COOP_WIDTH", &o->coop_width},
                {"SW_COOP_SKEW", &o->coop_skew},
                {"SW_INTRA_X2", &o->intra_x2},
                {"SW_INTRA_X2_RI", &o->intra_x2_rows},
                {"SW_INTRA_I16_FIRST", &o->intra_i16_first},
                {"SW_INTER_I16_SPAN", &o->inter_i16_span},
                {"SW_INT16_GUARD", &o->int16_guard},
                {"SW_RESCUE_STATS", &o->rescue_stats},
                {"SW_TAIL_PAIRS", &o->tail_pairs},
                {"SW_LPT_PERSIST", &o->lpt_persist},
                {"SW_LPT_ROWS", &o->lpt_rows},
                {"SW_TRI_WIDTH", &o->tri_width},
                {"SW_LPT_PIPE_TAIL", &o->lpt_pipe_tail},
                {"SW_DRAIN_SPIN", &o->drain_spin}};
    for (const auto& k : ints)
        if (const char* e = std::getenv(k.name); e && e[0]) *k.field = std::atoi(e);
    if (const char* e = std::getenv("SW_INTER_VARIANT"))
        std::snprintf(o->inter_variant, sizeof o->inter_variant, "%s", e);
    if (const char* e = std::getenv("SW_TRACE_FILE")) std::snprintf(o->trace_file, sizeof o->trace_file, "%s", e);
    return SW_OK;
}

int sw_set_opts(sw_handle* h, const sw_opts* o) {
    if (!h || !o) return fail(SW_E_INVALID, "null argument");
    if (o->size != static_cast<int32_t>(sizeof(sw_opts)))
        return fail(SW_E_INVALID, "sw_opts.size mismatch (initialise with sw_opts_init)");
    if (o->pair_group != -1 && o->pair_group != 2 && o->pair_group != 4)
        return fail(SW_E_INVALID, "sw_opts.pair_group must be -1, 2 or 4");
    h->opts = *o;
    h->opts.inter_variant[sizeof h->opts.inter_variant - 1] = 0;
    h->opts.trace_file[sizeof h->opts.trace_file - 1] = 0;
    return SW_OK;
}

int sw_get_opts(const sw_handle* h, sw_opts* o) {
    if (!h || !o) return fail(SW_E_INVALID, "null argument");
    *o = h->opts;
    return SW_OK;
}

int sw_set_stream(sw_handle* h, void* hip_stream) {
    if (!h) return fail(SW_E_INVALID, "null handle");
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    if (!h->own_stream) h->stream.release();  // the caller's
    h->own_stream = false;
    if (hip_stream) {
        h->stream = Stream(reinterpret_cast<hipStream_t>(hip_stream));  // borrowed (~sw_handle)
    } else {
        HIPCHECK(swk::stream_create(h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return SW_OK;
}

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

int sw_scan_device(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                   int32_t* scores_dev) {
    return scan_impl(h, db, query, qlen, sc, scores_dev);
}

int sw_scan(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
            int32_t* scores_host) {
    return scan_host(h, db, seq_src(query, qlen, sc), scores_host);
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

int sw_scan_pssm_device(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                        int32_t* scores_dev) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return scan_impl(h, db, pssm_src(p, gap_open, gap_extend), scores_dev);
}

int sw_scan_pssm_topk(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                      int32_t k, int64_t* keys_host) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return scan_topk_host(h, db, pssm_src(p, gap_open, gap_extend), k, keys_host);
}

namespace {
int check_batch(const int64_t* qoffsets, int32_t nq) {
    if (nq > 0 && qoffsets[0] < 0) return fail(SW_E_INVALID, "bad query offsets");
    for (int32_t k = 0; k < nq; ++k) {
        const int64_t ql = qoffsets[k + 1] - qoffsets[k];
        if (ql < 0 || ql > (int64_t(1) << 24)) return fail(SW_E_INVALID, "bad query offsets");
    }
    return SW_OK;
}
}  // namespace

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
        if ((rc = scan_impl(h, db, queries + qoffsets[k], static_cast<int32_t>(qoffsets[k + 1] - qoffsets[k]), sc,
                            scores_dev + k * n, k < last_scan)))
            return rc;
    // every tail has joined the handle's stream by now; join again in case a
    // scan above fell back to stream order after deferring an earlier one
    HIPCHECK(hipSetDevice(h->device));
    return join_tails(h);
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

namespace {
int read_events(const ScanEvents& se, sw_timing* t) {
    HIPCHECK(hipEventSynchronize(se.ev[3].get()));
    // intra runs on the side stream from the fork (ev0) to ev1; inter on the
    // main stream from ev0 to ev2; they overlap.
    // (events a scan did not record: the intra and inter spans fall back to
    // the whole scan, the cooperative kernel's to 0; a scan without a fork,
    // the merged launch, starts at ev6)
    auto has = [&](int k) { return (se.rec >> k & 1u) != 0; };
    const hipEvent_t start = has(0) ? se.ev[0].get() : se.ev[6].get();
    float t01 = 0, t02 = 0, t03 = 0;
    HIPCHECK(hipEventElapsedTime(&t03, start, se.ev[3].get()));
    t01 = t02 = t03;
    if (has(1)) HIPCHECK(hipEventElapsedTime(&t01, start, se.ev[1].get()));
    if (has(2)) HIPCHECK(hipEventElapsedTime(&t02, start, se.ev[2].get()));
    float t45 = 0, t67 = 0;
    if (has(4) && has(5)) HIPCHECK(hipEventElapsedTime(&t45, se.ev[4].get(), se.ev[5].get()));
    // (a merged launch that drains its own rescue lists ends the scan: ev[3])
    if (has(6)) HIPCHECK(hipEventElapsedTime(&t67, se.ev[6].get(), has(7) ? se.ev[7].get() : se.ev[3].get()));
    if (se.merged) {  // the merged launch: no separate intra span
        t01 = 0;
        t02 = t67;
    }
    t->intra_ms += t01;
    t->inter_ms += t02;
    t->total_ms += t03;
    t->coop_ms += t45;
    t->wave_ms += t67;
    t->launches += se.launches;
    return SW_OK;
}
}  // namespace

int sw_get_timing(sw_handle* h, sw_timing* out) {
    if (!h || !out) return fail(SW_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (!h->timed || h->nscans == 0) return SW_OK;
    return read_events(h->evpool[h->nscans - 1], out);
}

int sw_stream_wait_scan(sw_handle* h, void* hip_stream) {
    if (!h) return fail(SW_E_INVALID, "null handle");
    int rc;
    if ((rc = check_fault(h))) return rc;  // (a completed earlier scan's fault)
    if (!h->timed || h->nscans == 0) return SW_OK;  // no scan yet: nothing to wait for
    HIPCHECK(hipSetDevice(h->device));
    HIPCHECK(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), h->evpool[h->nscans - 1].ev[3].get(), 0));
    return SW_OK;
}

const char* sw_last_kernel(sw_handle* h) { return h ? h->last_kernel.c_str() : "none"; }
const char* sw_last_intra_kernel(sw_handle* h) { return h ? h->last_intra.c_str() : "none"; }

int sw_timing_reset(sw_handle* h) {
    if (!h) return fail(SW_E_INVALID, "null argument");
    h->nscans = 0;
    h->timed = false;
    return SW_OK;
}

int sw_timing_total(sw_handle* h, sw_timing* out, int32_t* nscans) {
    if (!h || !out || !nscans) return fail(SW_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    *nscans = static_cast<int32_t>(h->nscans);
    for (size_t k = 0; k < h->nscans; ++k) {
        int rc = read_events(h->evpool[k], out);
        if (rc) return rc;
    }
    return SW_OK;
}

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

int sw_scan_rank_device(sw_handle* h, const sw_db* cdb, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                        int32_t* scores_dev, int32_t k, const int32_t* gid_dev, int64_t id_base,
                        int64_t* keys_out_dev) {
    sw_db* db = const_cast<sw_db*>(cdb);
    if (!h || !db || !scores_dev || !keys_out_dev || k <= 0 || k > 4096)
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (!gid_dev && (id_base < 0 || id_base + db->max_id >= (int64_t(1) << 31)))
        return fail(SW_E_INVALID, "ids must fit in 31 bits");
    const RankReq rq{k, gid_dev, gid_dev ? 0 : id_base, keys_out_dev};
    return scan_impl(h, db, query, qlen, sc, scores_dev, false, &rq);
}

int sw_scan_topk(sw_handle* h, const sw_db* cdb, const uint8_t* query, int32_t qlen, const sw_scoring* sc, int32_t k,
                 int64_t* keys_host) {
    return scan_topk_host(h, cdb, seq_src(query, qlen, sc), k, keys_host);
}

}  // extern "C"

namespace {
// sw_align / sw_align_pssm: one traceback path; the forms differ in what is
// uploaded (the codes and the matrix, or nothing: the table is resident) and
// in the kernel's score functor (sw_align.hip).
int align_impl(sw_handle* h, const sw_db* cdb, const QuerySrc& src, const int32_t* ids, int32_t n,
               sw_alignment* out, char* ops, int64_t ops_stride) {
    sw_db* db = const_cast<sw_db*>(cdb);
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
    if (db->id_index.empty())
        for (int64_t k = 0; k < db->n; ++k) db->id_index.emplace(db->h_ids[k], k);
    std::vector<int64_t> sidx(n);
    for (int32_t k = 0; k < n; ++k) {
        auto it = db->id_index.find(ids[k]);
        if (it == db->id_index.end()) return fail(SW_E_INVALID, "sw_align: id not in the database");
        sidx[k] = it->second;
    }
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

// The hit table (sw_hits.hip): the rows of the pairs (query qidx[k], result
// id ids[k]), k in [0, n), into out[k]; qidx null: every pair is query 0's
// (sw_hit_stats, sw_scan_hits).  The queries are those of a batch
// (check_batch has passed).  What goes up, once: the queries, the matrix and
// one descriptor per hit (its query, where its subject is resident, its row);
// what comes down, once: the rows.  The hits launch in swplan::hits_order's
// order, longest wavefront first, in groups whose boundary rows fit the
// scratch budget; one synchronisation ends the call.
int hits_impl(sw_handle* h, const sw_db* cdb, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
              const sw_scoring* sc, const int32_t* qidx, const int32_t* ids, int64_t n, sw_hit* out) {
    sw_db* db = const_cast<sw_db*>(cdb);
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
    if (db->id_index.empty())
        for (int64_t k = 0; k < db->n; ++k) db->id_index.emplace(db->h_ids[k], k);
    if (db->pos_of.empty() && db->n > 0) {
        const std::vector<int64_t> order = swpack::length_order(db->h_offsets.data(), db->n);
        db->pos_of.resize(static_cast<size_t>(db->n));
        for (int64_t p = 0; p < db->n; ++p) db->pos_of[order[p]] = p;
    }
    // per pair, in the caller's order: the lengths, and the row as the host knows it
    std::vector<swk::HitDesc> hit(static_cast<size_t>(n));
    std::vector<int32_t> qlens(static_cast<size_t>(n));
    std::vector<int64_t> slens(static_cast<size_t>(n));
    int64_t work = 0;
    for (int64_t k = 0; k < n; ++k) {
        auto it = db->id_index.find(ids[k]);
        if (it == db->id_index.end()) return fail(SW_E_INVALID, "sw_hit_stats: id not in the database");
        const int64_t subj = it->second;
        const int32_t qi = qidx ? qidx[k] : 0;
        const swpack::Location loc = swpack::locate(db->pos_of[subj], db->shape.nlong);
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

// One query as a batch of one (sw_hit_stats, sw_scan_hits).
int hits_impl(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
              const int32_t* ids, int32_t n, sw_hit* out) {
    if (qlen < 0 || (qlen > 0 && !query)) return fail(SW_E_INVALID, "null argument");
    const int64_t offs[2] = {0, qlen};
    return hits_impl(h, db, query, offs, 1, sc, nullptr, ids, n, out);
}

// The batch's argument checks, shared by the three batch calls below.
int check_batch_args(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq) {
    if (!h || !db || nq < 0 || (nq > 0 && !qoffsets)) return fail(SW_E_INVALID, "null argument");
    if (int rc = check_batch(qoffsets, nq)) return rc;
    if (nq > 0 && qoffsets[nq] > qoffsets[0] && !queries) return fail(SW_E_INVALID, "null argument");
    return SW_OK;
}

// sw_scan_batch_topk: the scans back to back on the handle's stream, each
// with its ranking (RankReq: the top-K follows every stage that writes that
// query's scores, its rescue tail included, and the next scan's writes follow
// it in stream order), into keys[nq][k] behind ONE score row; one copy and
// one synchronisation end the call.
// hist_host (nullable, [nq][128][512]): every query's calibration table too,
// behind the keys in device memory, in the same copy sequence and
// synchronisation.
int batch_topk_impl(sw_handle* h, const sw_db* cdb, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                    const sw_scoring* sc, int32_t k, int64_t* keys_host, uint32_t* hist_host = nullptr) {
    sw_db* db = const_cast<sw_db*>(cdb);
    int rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    if (k <= 0 || k > 4096 || (nq > 0 && !keys_host)) return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    if (nq == 0) return SW_OK;
    const size_t nkeys = static_cast<size_t>(nq) * static_cast<size_t>(k);
    const size_t ntab = hist_host ? static_cast<size_t>(nq) * swcalib::kCells : 0;
    if (db->n == 0) {
        for (size_t i = 0; i < nkeys; ++i) keys_host[i] = INT64_MIN;
        if (hist_host) std::memset(hist_host, 0, ntab * sizeof(uint32_t));
        return SW_OK;
    }
    HIPCHECK(hipSetDevice(h->device));
    const size_t slots = static_cast<size_t>(db->max_id + 1);
    // the score row, then the nq x k keys, then the nq tables
    if ((rc = ensure_scores(h, slots + 2 * nkeys + 2 + ntab))) return rc;
    int64_t* keys_dev = reinterpret_cast<int64_t*>(h->d_scores.get() + round_up(static_cast<int64_t>(slots), 2));
    uint32_t* hist_dev = hist_host ? reinterpret_cast<uint32_t*>(keys_dev + nkeys) : nullptr;
    for (int32_t q = 0; q < nq; ++q) {
        const RankReq rq{k, nullptr, 0, keys_dev + static_cast<size_t>(q) * k};
        if ((rc = scan_impl(h, db, queries + qoffsets[q], static_cast<int32_t>(qoffsets[q + 1] - qoffsets[q]), sc,
                            h->d_scores.get(), false, &rq,
                            hist_dev ? hist_dev + static_cast<size_t>(q) * swcalib::kCells : nullptr)))
            return rc;
    }
    HIPCHECK(hipMemcpyAsync(keys_host, keys_dev, nkeys * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream.get()));
    if (hist_host)
        HIPCHECK(hipMemcpyAsync(hist_host, hist_dev, ntab * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHECK(hipStreamSynchronize(h->stream.get()));
    return check_fault(h);
}
}  // namespace

extern "C" {

int sw_hit_stats(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                 const int32_t* ids, int32_t n, sw_hit* out) {
    return hits_impl(h, db, query, qlen, sc, ids, n, out);
}

int sw_scan_batch_topk(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                       const sw_scoring* sc, int32_t k, int64_t* keys_host) {
    return batch_topk_impl(h, db, queries, qoffsets, nq, sc, k, keys_host);
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

}  // extern "C"

namespace {
// A scan's calibration from its table (sw_calib.h): the fit, and the
// zero-length subjects the table does not hold.
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

void calib_of(const sw_db* db, const uint32_t* hist, int32_t qlen, sw_calib* out) {
    swcalib::fit(hist, qlen, out);
    out->n_skipped = db->n - out->n_db;
}

// sw_scan_batch_hits; with_sig: its _sig form, the tables coming down with
// the keys, into sig ([nq][k]) and calib (nullable, [nq]).
int batch_hits_impl(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                    const sw_scoring* sc, int32_t k, sw_hit* out, int32_t* nhits, bool with_sig, sw_sig* sig,
                    sw_calib* calib) {
    if (!h || !db || !nhits || k <= 0 || k > 4096 || (nq > 0 && (!out || (with_sig && !sig))))
        return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    *nhits = 0;
    int rc;
    if ((rc = check_batch_args(h, db, queries, qoffsets, nq))) return rc;
    // first synchronisation: every query's keys (and table)
    std::vector<int64_t> keys(static_cast<size_t>(std::max(nq, 0)) * static_cast<size_t>(k));
    uint32_t* hist = nullptr;  // (pinned: the tables come down in the keys' synchronisation)
    if (with_sig && nq > 0 && (rc = ensure_hist_host(h, static_cast<size_t>(nq), &hist))) return rc;
    if ((rc = batch_topk_impl(h, db, queries, qoffsets, nq, sc, k, keys.data(), hist))) return rc;
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

// sw_scan_hits; sig (nullable, [k]) and calib (nullable): its _sig form.
int scan_hits_impl(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc, int32_t k,
                   sw_hit* out, int32_t* nhits, sw_sig* sig, sw_calib* calib) {
    if (!h || !db || !out || !nhits || k <= 0 || k > 4096) return fail(SW_E_INVALID, "bad argument (1 <= k <= 4096)");
    *nhits = 0;
    std::vector<int64_t> keys(static_cast<size_t>(k));
    uint32_t* hist = nullptr;
    if (sig)
        if (int rc = ensure_hist_host(h, 1, &hist)) return rc;
    if (int rc = scan_topk_host(h, db, seq_src(query, qlen, sc), k, keys.data(), hist)) return rc;
    const int32_t m = static_cast<int32_t>(std::min<int64_t>(k, db->n));
    std::vector<int32_t> ids(static_cast<size_t>(m));
    for (int32_t i = 0; i < m; ++i) ids[i] = static_cast<int32_t>(0x7fffffff - (keys[i] & 0xffffffffll));
    if (int rc = hits_impl(h, db, query, qlen, sc, ids.data(), m, out)) return rc;
    if (sig) {
        sw_calib c;
        calib_of(db, hist, qlen, &c);
        for (int32_t i = 0; i < m; ++i) swcalib::significance(c, out[i].score, out[i].s_len, &sig[i]);
        if (calib) *calib = c;
    }
    *nhits = m;
    return SW_OK;
}
}  // namespace

extern "C" {

int sw_scan_batch_hits(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                       const sw_scoring* sc, int32_t k, sw_hit* out, int32_t* nhits) {
    return batch_hits_impl(h, db, queries, qoffsets, nq, sc, k, out, nhits, false, nullptr, nullptr);
}

int sw_scan_batch_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* queries, const int64_t* qoffsets, int32_t nq,
                           const sw_scoring* sc, int32_t k, sw_hit* out, sw_sig* sig, int32_t* nhits,
                           sw_calib* calib) {
    return batch_hits_impl(h, db, queries, qoffsets, nq, sc, k, out, nhits, true, sig, calib);
}

int sw_scan_hits(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc, int32_t k,
                 sw_hit* out, int32_t* nhits) {
    return scan_hits_impl(h, db, query, qlen, sc, k, out, nhits, nullptr, nullptr);
}

int sw_scan_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                     int32_t k, sw_hit* out, sw_sig* sig, int32_t* nhits, sw_calib* calib) {
    if (!sig) return fail(SW_E_INVALID, "null argument");
    return scan_hits_impl(h, db, query, qlen, sc, k, out, nhits, sig, calib);
}

// ---- the calibration alone (sw_calib.h) -------------------------------------
int sw_score_hist_device(sw_handle* h, const sw_db* cdb, const int32_t* scores_dev, uint32_t* hist_dev) {
    sw_db* db = const_cast<sw_db*>(cdb);
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

int sw_scan_pssm_topk_calib(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                            int32_t k, int64_t* keys_host, sw_calib* calib) {
    if (!calib) return fail(SW_E_INVALID, "null argument");
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    if (!db) return fail(SW_E_INVALID, "null argument");
    uint32_t* hist = nullptr;
    if (int rc = ensure_hist_host(h, 1, &hist)) return rc;
    if (int rc = scan_topk_host(h, db, pssm_src(p, gap_open, gap_extend), k, keys_host, hist)) return rc;
    calib_of(db, hist, p->qlen, calib);
    return SW_OK;
}

int sw_align(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
             const int32_t* ids, int32_t n, sw_alignment* out, char* ops, int64_t ops_stride) {
    return align_impl(h, db, seq_src(query, qlen, sc), ids, n, out, ops, ops_stride);
}

int sw_align_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                  const int32_t* ids, int32_t n, sw_alignment* out, char* ops, int64_t ops_stride) {
    if (int rc = check_pssm(h, p, gap_open, gap_extend)) return rc;
    return align_impl(h, db, pssm_src(p, gap_open, gap_extend), ids, n, out, ops, ops_stride);
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
