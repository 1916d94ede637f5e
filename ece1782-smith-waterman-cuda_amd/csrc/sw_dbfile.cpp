// sw_dbfile.cpp — reading and writing the binary database file (sw_dbfile.h).
#include "sw_dbfile.h"

#include <cstdio>
#include <cstring>
#include <string>

#include "sw_kernels.h"  // swk::set_error, and through it sw_amd.h's codes

namespace swdbfile {

namespace {
constexpr char kDbMagic[8] = {'S', 'W', 'A', 'M', 'D', 'D', 'B', '1'};
struct DbFileHeader {
    char magic[8];
    int64_t n;         // subjects
    int64_t residues;  // total residue codes
    int32_t max_len;
    int32_t version;   // 1
    uint64_t fnv;      // FNV-1a 64 over offsets, ids and residues
};

uint64_t checksum(const std::vector<int64_t>& offs, const std::vector<int32_t>& ids, const std::vector<uint8_t>& res) {
    uint64_t f = kFnvBasis;
    f = fnv1a(f, offs.data(), offs.size() * sizeof(int64_t));
    f = fnv1a(f, ids.data(), ids.size() * sizeof(int32_t));
    return fnv1a(f, res.data(), res.size());
}
}  // namespace

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const auto* b = static_cast<const uint8_t*>(p);
    for (size_t k = 0; k < n; ++k) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

int write(const char* path, const std::vector<int64_t>& offs, const std::vector<int32_t>& ids,
          const std::vector<uint8_t>& res, int32_t max_len) {
    const int64_t n = static_cast<int64_t>(ids.size());
    DbFileHeader hd{};
    std::memcpy(hd.magic, kDbMagic, 8);
    hd.n = n;
    hd.residues = static_cast<int64_t>(res.size());
    hd.max_len = max_len;
    hd.version = 1;
    hd.fnv = checksum(offs, ids, res);
    FILE* fp = std::fopen(path, "wb");
    if (!fp) return swk::set_error(SW_E_IO, std::string("cannot open ") + path);
    bool ok = std::fwrite(&hd, sizeof hd, 1, fp) == 1 &&
              std::fwrite(offs.data(), sizeof(int64_t), offs.size(), fp) == offs.size() &&
              (n == 0 || std::fwrite(ids.data(), sizeof(int32_t), ids.size(), fp) == ids.size()) &&
              (res.empty() || std::fwrite(res.data(), 1, res.size(), fp) == res.size());
    ok = (std::fclose(fp) == 0) && ok;
    if (!ok) return swk::set_error(SW_E_IO, std::string("write failed: ") + path);
    return SW_OK;
}

int read(const char* path, std::vector<int64_t>& offs, std::vector<int32_t>& ids, std::vector<uint8_t>& res) {
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return swk::set_error(SW_E_IO, std::string("cannot open ") + path);
    DbFileHeader hd{};
    int rc = SW_OK;
    if (std::fread(&hd, sizeof hd, 1, fp) != 1 || std::memcmp(hd.magic, kDbMagic, 8) != 0 || hd.version != 1 ||
        hd.n < 0 || hd.residues < 0 || hd.n > (int64_t(1) << 40) || hd.residues > (int64_t(1) << 44)) {
        rc = swk::set_error(SW_E_IO, std::string("not a database file (sw_db_save format 1): ") + path);
    } else {
        try {
            offs.resize(hd.n + 1);
            ids.resize(hd.n);
            res.resize(static_cast<size_t>(hd.residues));
        } catch (...) {
            rc = swk::set_error(SW_E_NOMEM, "out of host memory");
        }
        if (!rc && (std::fread(offs.data(), sizeof(int64_t), offs.size(), fp) != offs.size() ||
                    (hd.n && std::fread(ids.data(), sizeof(int32_t), ids.size(), fp) != ids.size()) ||
                    (hd.residues && std::fread(res.data(), 1, res.size(), fp) != res.size())))
            rc = swk::set_error(SW_E_IO, std::string("truncated database file: ") + path);
    }
    std::fclose(fp);
    if (rc) return rc;
    if (checksum(offs, ids, res) != hd.fnv || offs.back() != hd.residues)
        return swk::set_error(SW_E_IO, std::string("database file checksum mismatch: ") + path);
    return SW_OK;
}

}  // namespace swdbfile
