// pssm_io_check.cpp — stand-alone program: sw_solver_write_pssm then
// sw_solver_read_pssm is the identity on the rows and on the consensus
// (include/sw_solver_ext.h).  Built by tests/test_profile_cpu.py from
// csrc/swsolver.cpp against lib/libswamd.so; argv[1] is a directory to write
// in.  The table is rows[i][c] = (31 i + 17 c) mod 201 - 100 over 60 positions,
// consensus letter i mod 25 (the Python test reads the file back too).
// Prints "pssm_io_check ok".
#include <cstdio>
#include <string>
#include <vector>

#include "sw_solver_ext.h"

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";
    const int n = 60;
    std::vector<int8_t> rows(n * 25);
    std::string cons;
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 25; ++c) rows[i * 25 + c] = static_cast<int8_t>((31 * i + 17 * c) % 201 - 100);
        cons += kLetters[i % 25];
    }
    std::string err;
    CHECK(sw_solver_write_pssm(dir + "/table.pssm", rows, cons, &err));
    std::vector<int8_t> back;
    std::string cback;
    CHECK(sw_solver_read_pssm(dir + "/table.pssm", &back, &cback, &err));
    CHECK(back == rows);
    CHECK(cback == cons);

    // no consensus given: the best column, first in code order, as the reader picks it without a letter
    CHECK(sw_solver_write_pssm(dir + "/best.pssm", rows, std::string(), &err));
    CHECK(sw_solver_read_pssm(dir + "/best.pssm", &back, &cback, &err));
    CHECK(back == rows);
    for (int i = 0; i < n; ++i) {
        int best = 0;
        for (int c = 1; c < 25; ++c)
            if (rows[i * 25 + c] > rows[i * 25 + best]) best = c;
        CHECK(cback[i] == kLetters[best]);
    }
    // lower case and bytes outside the alphabet: as the encoder reads them
    std::vector<int8_t> two(rows.begin(), rows.begin() + 50);
    CHECK(sw_solver_write_pssm(dir + "/two.pssm", two, "a/", &err));
    CHECK(sw_solver_read_pssm(dir + "/two.pssm", &back, &cback, &err));
    CHECK(back == two && cback == "A*");

    // what cannot be written
    CHECK(!sw_solver_write_pssm(dir + "/bad.pssm", std::vector<int8_t>(), cons, &err) && !err.empty());
    CHECK(!sw_solver_write_pssm(dir + "/bad.pssm", std::vector<int8_t>(26, 0), std::string(), &err));
    CHECK(!sw_solver_write_pssm(dir + "/bad.pssm", two, "A", &err));
    CHECK(!sw_solver_write_pssm(dir + "/bad.pssm", std::vector<int8_t>(25, 101), std::string(), &err));
    CHECK(!sw_solver_write_pssm(dir + "/no/such/dir/x.pssm", two, "AR", &err));

    if (failures) return 1;
    std::printf("pssm_io_check ok\n");
    return 0;
}
