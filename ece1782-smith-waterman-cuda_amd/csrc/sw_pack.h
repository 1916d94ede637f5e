// sw_pack.h — the packed database layout as pure host code (sw_pack.cpp): no
// HIP call, no handle, so the layout every scan kernel, sw_synth_fill_* and
// sw_align decode is checked on the CPU (tests/native/pack_check.cpp).
// sw_db.cpp's build_db asks for a Shape, allocates, and uploads what
// fill_block / fill_long write:
//   * subjects longest first, stable (file order within a length);
//   * those longer than the threshold one after another, each start 64-byte
//     aligned (the wavefront kernels' part);
//   * the rest dealt 64 to a block, a block being groups of [64 lanes][16
//     codes] as wide as its longest subject (the inter kernels' part);
//   * every byte stored as swk::kStored of its code, swk::kPadCode past a
//     subject's end.
#pragma once

#include <cstdint>
#include <vector>

namespace swpack {

// The subjects to pack, read-only: subject k holds residues
// [offsets[k], offsets[k + 1]) and reports its score as ids[k].
struct Subjects {
    int64_t n = 0;
    const int64_t* offsets = nullptr;   // [n + 1]
    const int32_t* ids = nullptr;       // [n]
    const uint8_t* residues = nullptr;  // null: a synthetic database (filled on the device)
    int64_t len(int64_t k) const { return offsets[k + 1] - offsets[k]; }
};

// Subject indices sorted by length, longest first, stable (file order
// within a length): a counting sort when lengths are bounded, else
// std::stable_sort.
std::vector<int64_t> length_order(const int64_t* offs, int64_t n);

// One packed layout: what a long threshold makes of the subjects.
struct Shape {
    std::vector<int64_t> order;        // [n] subjects, longest first
    // intra (long) part: subjects order[0 .. nlong)
    int64_t nlong = 0;
    std::vector<uint64_t> loff;        // [nlong + 1] byte offset of each, 64-byte aligned; the last = ltotal
    std::vector<int32_t> llen, lid;    // [nlong] length and result id
    uint64_t ltotal = 0;               // bytes of the long part
    int32_t long_max = 0;              // the longest long subject (0: none)
    // inter part: block b holds subjects order[nlong + 64 b ...), one per lane
    int64_t nblocks = 0;
    std::vector<uint64_t> blk_off;     // [nblocks + 1] byte offset of each block's group 0; the last = total
    std::vector<uint32_t> blk_groups;  // [nblocks] 16-column groups, widest first
    std::vector<uint32_t> blk_cols;    // [nblocks] the longest subject rounded up to 8 columns
    std::vector<int32_t> lane_ids;     // [nblocks][64] result id, -1 = empty lane
    std::vector<int32_t> lane_len;     // [nblocks][64] length, 0 = empty lane (want_lane_len only)
    std::vector<int64_t> blk_res;      // [nblocks] unpadded residues
    uint64_t total = 0;                // bytes of the inter part: one per scanned (lane, column)

    // Drop what only the upload reads (the order, the offsets, the lane
    // tables); the counts and blk_groups, blk_res, llen stay for the scans.
    void release_upload_tables();
};

Shape plan(const Subjects& s, int32_t long_threshold, bool want_lane_len);

// Where the subject at position p of the length order (Shape::order[p]) lies
// in a layout with nlong long subjects: long slot p (lane = -1), or lane
// (p - nlong) % 64 of block (p - nlong) / 64.  Only nlong depends on the long
// threshold, so a position survives a re-pack.  Residue j of the subject is
// byte swk::hit_residue_at(lane, j) from loff[slot] / blk_off[slot]
// (sw_hits.hip reads it there).
struct Location {
    int64_t slot;
    int32_t lane;
};
Location locate(int64_t p, int64_t nlong);

// Block b's bytes, all blk_groups[b] * kGroupBytes of them, padding included.
void fill_block(const Subjects& s, const Shape& sh, int64_t b, uint8_t* dst);
// Long subject k's bytes, all loff[k + 1] - loff[k] of them, padding included.
void fill_long(const Subjects& s, const Shape& sh, int64_t k, uint8_t* dst);

}  // namespace swpack
