// sw_cli.h — main's command line as data: the flags, their values and every
// check that is made before a file is read.  Pure: nothing of the library and
// of no GPU runtime (tests/native/cli_opts_check.cpp links sw_cli.cpp alone).
#ifndef SW_CLI_H
#define SW_CLI_H

#include <string>

namespace swcli {

// One flag as given: its text, and the number the flag table's rule reads
// from it (ok: the text is such a number).  The last of a repeated flag wins.
struct Value {
    bool set = false;
    std::string text;
    bool ok = false;
    long i = 0;
    double d = 0;
};

struct Options {
    bool help = false;
    Value query, pssm, queries, db, make_db, gpus, matrix, gap_open, gap_extend, topk, hits, evalue, rank, max_evalue,
        metrics_json, iterations, inclusion_evalue, write_pssm;

    // the scoring is the reference's unless one of its flags is given
    bool custom() const { return matrix.set || gap_open.set || gap_extend.set; }
    int gap_open_cost() const { return gap_open.set ? static_cast<int>(gap_open.i) : 2; }
    int gap_extend_cost() const { return gap_extend.set ? static_cast<int>(gap_extend.i) : gap_open_cost(); }
    bool ranked() const { return rank.set; }
    // the iterated search: its report's size and its inclusion threshold
    int iter_topk() const { return topk.set ? static_cast<int>(topk.i) : 500; }
    double iter_inclusion() const { return inclusion_evalue.set ? inclusion_evalue.d : 1e-3; }
    // a .swdb file (sw_db_save) in the place of a FASTA database
    bool binary_db() const {
        return db.text.size() > 5 && db.text.compare(db.text.size() - 5, 5, ".swdb") == 0;
    }
};

// What main does next.  STOP: write `err` to stderr, the usage to stdout when
// `usage`, and exit with `code`.  after_matrix: the check that failed comes
// after the --matrix file has been read, whose own error goes first.
struct Verdict {
    enum What { PROCEED, MAKE_DB, STOP } what = PROCEED;
    int code = 0;
    std::string err;
    bool usage = false;
    bool after_matrix = false;
};

const char* usage_text();
// argv into *o, in order; STOP at the first argument that is no flag, lacks
// its value or is unknown.
Verdict parse(int argc, const char* const* argv, Options* o);
// Every check of the flags against each other and of their values, in the
// order main has always made them: the first that fails is the one reported.
Verdict validate(const Options& o);

}  // namespace swcli

#endif  // SW_CLI_H
