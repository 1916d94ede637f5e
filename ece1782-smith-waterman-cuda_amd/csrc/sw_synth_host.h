// sw_synth_host.h — the host half of the synthetic generator (SURVEY.md §8d
// config C4; the device half is sw_synth.hip): the length and residue tables,
// and any subject's length and residues from (seed, global id).
//   length(id)     = len[h(seed, id, LEN_SALT) >> 52]              (4096 log-normal quantiles)
//   residue(id, j) = lut[(h(seed, id, j >> 2) >> (16 * (j & 3))) & 0xffff]
// with h = swk::syn_hash (sw_synth_hash.h).
#pragma once

#include <cstdint>

namespace swk {

// Swiss-Prot composition (percent), codes 0..19 = A R N D C Q E G H I L K M F
// P S T W Y V (the same table as synth.py): the generator's residue
// frequencies, and the background of the profile builder (sw_pssm_build.cpp).
inline constexpr double kSwissProtFreq[20] = {8.25, 5.53, 4.06, 5.45, 1.37, 3.93, 6.75, 7.07, 2.27, 5.96,
                                              9.66, 5.84, 2.42, 3.86, 4.70, 6.56, 5.34, 1.08, 2.92, 6.87};

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
