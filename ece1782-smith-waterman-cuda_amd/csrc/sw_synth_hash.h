// sw_synth_hash.h — the synthetic generator's counter-based hash, shared by
// the device fill (sw_synth.hip) and its host half (sw_synth_host.cpp):
//   h(seed, id, k) = mix(seed * G1 + mix(id * G2 + k))         (splitmix64 mix)
// Integer-only, so the host and any CPU restatement reproduce it bit for bit
// (synth.py counter_* functions, tests/test_synth_counter.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swk {

__host__ __device__ inline uint64_t syn_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ inline uint64_t syn_hash(uint64_t seed, uint64_t id, uint64_t k) {
    return syn_mix(seed * 0x9E3779B97F4A7C15ull + syn_mix(id * 0xD6E8FEB86659FD93ull + k));
}

}  // namespace swk
