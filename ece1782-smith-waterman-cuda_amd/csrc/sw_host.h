// sw_host.h — what the host driver (sw_driver.h's units, sw_group.cpp) shares and no
// kernel sees: the owners of HIP resources, their allocation helpers and the
// error macro.  A HIP resource is a member or a local of owner type and is
// released by its destructor; a raw pointer, event or stream is an alias
// into something an owner holds, and says so where it is declared.
#pragma once

#include <hip/hip_runtime.h>

#include "sw_kernels.h"  // swk::set_error, and through it sw_amd.h's codes
#include "sw_owned.h"

// A failed HIP call returns SW_E_HIP from the calling function, with its text as sw_last_error().
#define HIPCHECK(expr)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return swk::set_error(SW_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

namespace swk {

template <class T, hipError_t (*Free)(void*)>
void mem_free(T* p) { (void)Free(p); }
inline void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }

template <class T>
using DevPtr = Owned<T*, mem_free<T, hipFree>>;       // device memory
template <class T>
using HostPtr = Owned<T*, mem_free<T, hipHostFree>>;  // pinned or mapped host memory
using Event = Owned<hipEvent_t, event_destroy>;
using Stream = Owned<hipStream_t, stream_destroy>;

// Each releases what the owner held, then creates: a buffer that grows never
// holds the old and the new allocation at once.  The owner is empty after a
// failure.
template <class O, class F>
hipError_t recreate(O& o, F&& create) {
    o.reset();
    decltype(o.get()) raw{};
    const hipError_t e = create(&raw);
    if (e == hipSuccess) o = O(raw);
    return e;
}
template <class T>
hipError_t dev_alloc(DevPtr<T>& p, size_t bytes) {
    return recreate(p, [&](T** raw) { return hipMalloc(reinterpret_cast<void**>(raw), bytes); });
}
template <class T>
hipError_t host_alloc(HostPtr<T>& p, size_t bytes, unsigned flags) {
    return recreate(p, [&](T** raw) { return hipHostMalloc(reinterpret_cast<void**>(raw), bytes, flags); });
}
inline hipError_t event_create(Event& ev, unsigned flags = hipEventDefault) {
    return recreate(ev, [&](hipEvent_t* raw) { return hipEventCreateWithFlags(raw, flags); });
}
inline hipError_t stream_create(Stream& s, unsigned flags) {
    return recreate(s, [&](hipStream_t* raw) { return hipStreamCreateWithFlags(raw, flags); });
}
inline hipError_t stream_create(Stream& s, unsigned flags, int priority) {
    return recreate(s, [&](hipStream_t* raw) { return hipStreamCreateWithPriority(raw, flags, priority); });
}

}  // namespace swk
