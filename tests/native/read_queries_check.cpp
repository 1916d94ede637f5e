// tests/native/read_queries_check.cpp — prints what sw_solver_read_queries
// (include/sw_solver_ext.h) makes of the file named on the command line, for
// tests/test_batch_hits_cpu.py: "records <n>" and one "<name>|<length>|<residues>"
// line per record, or "error: <message>" and exit status 1.  No GPU is touched.
#include <cstdio>
#include <string>
#include <vector>

#include "sw_solver_ext.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<std::string> names, seqs;
    std::string err;
    if (!sw_solver_read_queries(argv[1], &names, &seqs, &err)) {
        std::printf("error: %s\n", err.c_str());
        return 1;
    }
    std::printf("records %zu\n", seqs.size());
    for (size_t k = 0; k < seqs.size(); ++k) std::printf("%s|%zu|%s\n", names[k].c_str(), seqs[k].size(), seqs[k].c_str());
    return names.size() == seqs.size() ? 0 : 2;
}
