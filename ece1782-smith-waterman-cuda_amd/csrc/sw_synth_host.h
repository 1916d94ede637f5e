// sw_synth_host.h — the host half of the synthetic generator (SURVEY.md §8d
// config C4; the device half is sw_synth.hip): the length and residue tables,
// and any subject's length and residues from (seed, global id).
//   length(id)     = len[h(seed, id, LEN_SALT) >> 52]              (4096 log-normal quantiles)
//   residue(id, j) = lut[(h(seed, id, j >> 2) >> (16 * (j & 3))) & 0xffff]
// with h = swk::syn_hash (sw_synth_hash.h).
#pragma once

#include <cstdint>

namespace swk {

struct SynthTables {
    int32_t len[4096];     // log-normal length quantiles: median 290, sigma 0.657, in [5, 35213]
    uint8_t lut[65536];    // uniform u16 -> residue code
    uint8_t lut_stored[65536];  // ... as stored on the device (swk::kStored)
    SynthTables();
};
const SynthTables& synth_tables();

int32_t synth_length(uint64_t seed, uint64_t gid);
// out[0 .. L): subject gid's residue codes.
void synth_residues(uint64_t seed, uint64_t gid, int64_t L, uint8_t* out);

}  // namespace swk
