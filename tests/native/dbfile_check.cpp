// tests/native/dbfile_check.cpp — CPU check of the binary database file
// (sw_dbfile.cpp): what write() stores read() gives back, and a file that is
// cut, altered or not of this format is refused with the code and message
// sw_db_load has always reported.  Linked from sw_dbfile.cpp alone: the
// error sink swk::set_error (sw_handle.cpp's in the library) is this file's.
// usage: dbfile_check SCRATCH_DIR.  Built and run by tests/test_dbfile.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sw_dbfile.h"
#include "sw_kernels.h"

static int failures = 0;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++failures;                        \
        }                                      \
    } while (0)

static int g_code = 0;
static std::string g_msg;
int swk::set_error(int code, const std::string& msg) {
    g_code = code;
    g_msg = msg;
    return code;
}

typedef std::vector<uint8_t> Bytes;

static Bytes slurp(const std::string& path) {
    Bytes b;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        int ch;
        while ((ch = std::fgetc(f)) != EOF) b.push_back(static_cast<uint8_t>(ch));
        std::fclose(f);
    }
    return b;
}

static void spit(const std::string& path, const Bytes& b) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (f && !b.empty()) std::fwrite(b.data(), 1, b.size(), f);
    if (f) std::fclose(f);
}

struct Db {
    std::vector<int64_t> offs;
    std::vector<int32_t> ids;
    Bytes res;
};

// read() of `bytes` fails with `code` and a message starting with `prefix` and naming the file
static void refused(const char* what, const std::string& path, const Bytes& bytes, int code, const char* prefix) {
    spit(path, bytes);
    Db d;
    g_code = 0;
    g_msg.clear();
    const int rc = swdbfile::read(path.c_str(), d.offs, d.ids, d.res);
    CHECK(rc == code && g_code == code && g_msg == std::string(prefix) + path, "%s: rc %d \"%s\", want %d \"%s...\"",
          what, rc, g_msg.c_str(), code, prefix);
    std::printf("%s: %d %s\n", what, rc, g_msg.substr(0, g_msg.size() - path.size()).c_str());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1], path = dir + "/db.bin", bad = dir + "/bad.bin";

    // ---- round trips: subjects of 3, 0 and 5 residues, custom ids; and no subject at all
    Db a;
    a.offs = {0, 3, 3, 8};
    a.ids = {7, 1000000, 0};
    a.res = {0, 24, 11, 5, 6, 7, 8, 9};
    for (const Db& d : {a, Db{{0}, {}, {}}}) {
        const char* what = d.ids.empty() ? "round-trip-empty" : "round-trip";
        CHECK(swdbfile::write(path.c_str(), d.offs, d.ids, d.res, d.ids.empty() ? 0 : 5) == SW_OK, "%s: write: %s",
              what, g_msg.c_str());
        const size_t want = 40 + 8 * d.offs.size() + 4 * d.ids.size() + d.res.size();
        CHECK(slurp(path).size() == want, "%s: %zu bytes on disk, want %zu", what, slurp(path).size(), want);
        Db r;
        r.offs = {99};  // what the caller's vectors held is replaced
        CHECK(swdbfile::read(path.c_str(), r.offs, r.ids, r.res) == SW_OK, "%s: read: %s", what, g_msg.c_str());
        CHECK(r.offs == d.offs && r.ids == d.ids && r.res == d.res, "%s: read differs from what was written", what);
        std::printf("%s: %zu subjects, %zu bytes\n", what, r.ids.size(), want);
    }
    CHECK(swdbfile::write(path.c_str(), a.offs, a.ids, a.res, 5) == SW_OK, "write: %s", g_msg.c_str());
    const Bytes good = slurp(path);
    // header 40 bytes: magic 0, n 8, residues 16, max_len 24, version 28, fnv 32
    const size_t o_offs = 40, o_ids = o_offs + 8 * 4, o_res = o_ids + 4 * 3;
    CHECK(good.size() == o_res + 8 && std::memcmp(good.data(), "SWAMDDB1", 8) == 0 && good[8] == 3 && good[16] == 8 &&
              good[24] == 5 && good[28] == 1,
          "the header's fields are not where format 1 puts them");
    if (failures) return 1;

    // ---- a file cut inside each section
    const struct {
        const char* what;
        size_t keep;
        const char* prefix;
    } cuts[] = {{"cut-in-header", 20, "not a database file (sw_db_save format 1): "},
                {"cut-in-offsets", o_offs + 12, "truncated database file: "},
                {"cut-in-ids", o_ids + 6, "truncated database file: "},
                {"cut-in-residues", o_res + 3, "truncated database file: "},
                {"cut-at-residues", o_res, "truncated database file: "}};
    for (const auto& c : cuts) refused(c.what, bad, Bytes(good.begin(), good.begin() + c.keep), SW_E_IO, c.prefix);

    // ---- one flipped byte in each payload section, and in the checksum itself
    const struct {
        const char* what;
        size_t at;
    } flips[] = {{"flip-in-offsets", o_offs + 8}, {"flip-in-ids", o_ids + 5}, {"flip-in-residues", o_res + 7},
                 {"flip-in-checksum", 33}};
    for (const auto& f : flips) {
        Bytes b = good;
        b[f.at] ^= 0x04;
        refused(f.what, bad, b, SW_E_IO, "database file checksum mismatch: ");
    }

    // ---- not this format
    auto with = [&](size_t at, std::vector<uint8_t> v) {
        Bytes b = good;
        std::copy(v.begin(), v.end(), b.begin() + at);
        return b;
    };
    const char* notdb = "not a database file (sw_db_save format 1): ";
    refused("bad-magic", bad, with(7, {'2'}), SW_E_IO, notdb);
    refused("version-2", bad, with(28, {2}), SW_E_IO, notdb);
    refused("negative-n", bad, with(8, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff}), SW_E_IO, notdb);
    refused("negative-residues", bad, with(16, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff}), SW_E_IO, notdb);
    refused("empty-file", bad, Bytes(), SW_E_IO, notdb);
    // the header's residue count one less than offsets[n]: a file of that
    // many residues whose checksum is right for what it holds
    {
        Bytes b(good.begin(), good.end() - 1);
        b[16] = 7;
        uint64_t f = swdbfile::fnv1a(swdbfile::kFnvBasis, b.data() + o_offs, b.size() - o_offs);
        std::memcpy(b.data() + 32, &f, 8);
        refused("residues-disagree-with-offsets", bad, b, SW_E_IO, "database file checksum mismatch: ");
    }
    {
        Db d;
        g_code = 0;
        const std::string gone = dir + "/no-such-dir/db.bin";
        CHECK(swdbfile::read(gone.c_str(), d.offs, d.ids, d.res) == SW_E_IO && g_msg == "cannot open " + gone,
              "missing file: \"%s\"", g_msg.c_str());
        CHECK(swdbfile::write(gone.c_str(), a.offs, a.ids, a.res, 5) == SW_E_IO && g_msg == "cannot open " + gone,
              "unwritable path: \"%s\"", g_msg.c_str());
    }
    // FNV-1a 64 of "a" from the published offset basis (the published test vector)
    CHECK(swdbfile::fnv1a(14695981039346656037ull, "a", 1) == 0xaf63dc4c8601ec8cull, "fnv1a(\"a\")");
    if (failures) {
        std::printf("dbfile_check: %d failures\n", failures);
        return 1;
    }
    std::printf("dbfile_check ok\n");
    return 0;
}
