// sw_handle.cpp — the handle of the host driver (sw_driver.h): the error
// sink, sw_create / sw_destroy and the streams, the kernel-form overrides
// (sw_opts), the fault word, and the scans' event sets and timing.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "sw_driver.h"

using namespace swd;

namespace {

thread_local std::string g_err;

// Faults reported so far (any handle): a drain that gave up on an entry
// left claimed entries of its database's rescue lists un-reset, so every
// database re-initialises its lists at its first scan after a fault
// (sw_db::list_epoch) and later scans are exact again.
std::atomic<uint64_t> g_fault_epoch{0};

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

int swk::set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

sw_opts swd::default_opts() {
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

uint64_t swd::fault_epoch() { return g_fault_epoch.load(); }

// (sw_kernels.h list_wait_take sets the word: fail loudly, once)
int swd::check_fault(sw_handle* h) {
    if (h && h->h_fault.get() && __atomic_load_n(h->h_fault.get(), __ATOMIC_ACQUIRE)) {
        __atomic_store_n(h->h_fault.get(), 0, __ATOMIC_RELEASE);
        g_fault_epoch.fetch_add(1);
        return fail(SW_E_DEVICE, "sw_scan_lpt: a claimed rescue-list entry never appeared; the handle's scans "
                                 "since the last successful call may hold unrescued scores");
    }
    return SW_OK;
}

// (before a release, or after a failed scan; the first error, for the callers that check)
hipError_t swd::quiesce(sw_handle* h) {
    hipError_t first = hipSuccess;
    for (hipStream_t st : {h->stream.get(), h->side.get(), h->side2.get(), h->tail.get()})
        if (st) {
            const hipError_t e = hipStreamSynchronize(st);
            if (first == hipSuccess) first = e;
        }
    return first;
}

// What completes on the handle's stream afterwards (a non-deferred scan, the
// end of a batch) includes the rescued scores of the scans before it.
int swd::join_tails(sw_handle* h) {
    for (int q = 0; q < 2; ++q)
        if (h->tail_pending[q]) {
            HIPCHECK(hipStreamWaitEvent(h->stream.get(), h->tail_done[q].get(), 0));
            h->tail_pending[q] = false;
        }
    return SW_OK;
}

int swd::next_events(sw_handle* h) {
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

extern "C" {

const char* sw_last_error(void) { return g_err.c_str(); }

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

}  // extern "C"
