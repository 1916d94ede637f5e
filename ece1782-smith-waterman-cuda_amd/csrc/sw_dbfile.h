// sw_dbfile.h — the binary database file, format
// "SWAMDDB1", as pure host code (sw_dbfile.cpp; tests/native/dbfile_check.cpp):
//   header   : magic, n, residues, max_len, version 1, FNV-1a 64 of the rest
//   offsets  : int64 [n + 1]
//   ids      : int32 [n]
//   residues : uint8 [residues]
// sw_db_save writes the subjects longest first with their result ids, so
// loading gives identical scores[id].  Both functions return an SW_E_* code
// and leave its text with swk::set_error.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace swdbfile {

// Where format 1's checksum starts (the published FNV offset basis less its
// last digit: part of the format now).
constexpr uint64_t kFnvBasis = 1469598103934665603ull;
// FNV-1a 64 of p[0 .. n) continued from h.
uint64_t fnv1a(uint64_t h, const void* p, size_t n);

int write(const char* path, const std::vector<int64_t>& offsets, const std::vector<int32_t>& ids,
          const std::vector<uint8_t>& residues, int32_t max_len);
// The file's subjects: offsets.size() - 1 of them.
int read(const char* path, std::vector<int64_t>& offsets, std::vector<int32_t>& ids, std::vector<uint8_t>& residues);

}  // namespace swdbfile
