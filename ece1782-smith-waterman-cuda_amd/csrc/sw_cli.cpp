// sw_cli.cpp — main's flags and their checks (sw_cli.h).  The messages and
// their precedence are main's contract: tests/golden/cli_flag_cases.json pins
// them, recorded before this unit existed.
#include "sw_cli.h"

#include <cstdint>
#include <cstdlib>
#include <initializer_list>

namespace swcli {

namespace {

// How a flag's value is read.  FLAG takes none ("--evalue"; "--evalue=x" is
// accepted and x dropped); INT is a whole-string integer in [lo, hi]; COUNT is
// atoi's reading, as --gpus has always been read ("2x" is 2, "x" is 0);
// POSITIVE a whole-string number > 0.
enum Kind { FLAG, TEXT, INT, COUNT, POSITIVE };

struct Flag {
    const char* name;
    Kind kind;
    Value Options::*at;
    long lo, hi;
};

const Flag kFlags[] = {
    {"query", TEXT, &Options::query, 0, 0},
    {"pssm", TEXT, &Options::pssm, 0, 0},
    {"queries", TEXT, &Options::queries, 0, 0},
    {"db", TEXT, &Options::db, 0, 0},
    {"make-db", TEXT, &Options::make_db, 0, 0},
    {"gpus", COUNT, &Options::gpus, 0, 0},
    {"matrix", TEXT, &Options::matrix, 0, 0},
    {"gap-open", INT, &Options::gap_open, 1, 1000},
    {"gap-extend", INT, &Options::gap_extend, 1, 1000},
    {"topk", INT, &Options::topk, 1, INT32_MAX},
    {"hits", INT, &Options::hits, 1, 4096},
    {"evalue", FLAG, &Options::evalue, 0, 0},
    {"rank", TEXT, &Options::rank, 0, 0},
    {"max-evalue", POSITIVE, &Options::max_evalue, 0, 0},
    {"metrics-json", FLAG, &Options::metrics_json, 0, 0},
    {"iterations", INT, &Options::iterations, 1, 1000},
    {"inclusion-evalue", POSITIVE, &Options::inclusion_evalue, 0, 0},
    {"write-pssm", TEXT, &Options::write_pssm, 0, 0},
};

const Flag* find_flag(const std::string& name) {
    for (const Flag& f : kFlags)
        if (name == f.name) return &f;
    return nullptr;
}

Value read_value(const Flag& f, const std::string& text) {
    Value v;
    v.set = true;
    v.text = text;
    char* end = nullptr;
    switch (f.kind) {
    case INT:
        v.i = std::strtol(text.c_str(), &end, 10);
        v.ok = !text.empty() && *end == '\0' && v.i >= f.lo && v.i <= f.hi;
        break;
    case COUNT:
        v.i = std::atoi(text.c_str());
        v.ok = true;
        break;
    case POSITIVE:
        v.d = std::strtod(text.c_str(), &end);
        v.ok = !text.empty() && *end == '\0' && v.d > 0;
        break;
    case FLAG:
    case TEXT:
        v.ok = true;
        break;
    }
    return v;
}

Verdict stop(const std::string& err, bool usage = false) {
    Verdict v;
    v.what = Verdict::STOP;
    v.code = 1;
    v.err = err;
    v.usage = usage;
    return v;
}

// The word of the first given flag of a "cannot be combined with" list
// (--gpus 1 is no conflict), or null.
struct With {
    const Value& flag;
    const char* word;
};
const char* first_of(const Options& o, std::initializer_list<With> list) {
    for (const With& w : list)
        if (w.flag.set && (&w.flag != &o.gpus || w.flag.i != 1)) return w.word;
    return nullptr;
}

}  // namespace

// (The text is pinned by tests/golden/cli_flag_cases.json; --iterations,
// --inclusion-evalue and --write-pssm are described in main.cpp and README.md.)
const char* usage_text() {
    return "Smith-Waterman MI355X Usage:\n"
           "  --help                Display this help message\n"
           "  --query arg           Path to query file (required, or --pssm)\n"
           "  --pssm arg            Path to a PSSM text file, in the place of --query\n"
           "  --queries arg         Path to a multi-record FASTA file of queries, in the place of --query;\n"
           "                        needs --hits K or --topk K (1..4096): one block of output per query\n"
           "  --db arg              Path to database file (required; FASTA, or a .swdb file)\n"
           "  --make-db arg         Write the FASTA --db as a binary .swdb database and exit\n"
           "  --gpus arg            Shard the FASTA database over this many GPUs (default 1)\n"
           "  --matrix arg          blosum50 (default, the reference's), blosum62, or a matrix file\n"
           "  --gap-open arg        Cost of a gap's first residue (default 2)\n"
           "  --gap-extend arg      Cost of each further gap residue (default: --gap-open, linear)\n"
           "  --topk arg            Print only the arg best subjects (score desc, id asc)\n"
           "  --hits arg            Print the arg best subjects (1..4096) as a hit table: id score q_begin\n"
           "                        q_end s_begin s_end s_len length identities positives gap_opens gaps\n"
           "  --evalue              With --hits: append evalue and bits to each row (calibrated on the\n"
           "                        scan's own scores) and print a '# calibration' line per query\n"
           "  --rank arg            evalue: with --hits K --evalue, rank by E-value instead of raw score and\n"
           "                        print a '# significant N shown M' line per query\n"
           "  --max-evalue arg      With --rank evalue: only subjects with an E-value of at most arg (> 0)\n";
}

Verdict parse(int argc, const char* const* argv, Options* o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--help") {
            o->help = true;
            continue;
        }
        if (a.rfind("--", 0) != 0) return stop("", true);
        std::string key = a.substr(2), val;
        const size_t eq = key.find('=');
        const Flag* f = find_flag(key.substr(0, eq));
        if (eq != std::string::npos) {
            val = key.substr(eq + 1);
            key = key.substr(0, eq);
        } else if (!f || f->kind != FLAG) {
            if (i + 1 >= argc) return stop("", true);
            val = argv[++i];
        }
        if (!f) return stop("unrecognised option '--" + key + "'\n");
        o->*(f->at) = read_value(*f, val);
    }
    return Verdict();
}

Verdict validate(const Options& o) {
    if (!o.help) {  // each of these is made before any file is read
        if (o.evalue.set && !o.hits.set) return stop("--evalue needs --hits K: it adds columns to the hit table\n");
        if (o.rank.set) {
            if (o.rank.text != "evalue") return stop("--rank takes one value: evalue\n");
            if (!o.evalue.set || !o.hits.set)
                return stop("--rank evalue needs --hits K --evalue: it orders the hit table by its evalue column\n");
        }
        if (o.iterations.set) {
            if (!o.iterations.ok) return stop("--iterations must be an integer in 1..1000\n");
            if (const char* with = first_of(o, {{o.pssm, "--pssm"}, {o.queries, "--queries"}, {o.hits, "--hits"},
                                                {o.gpus, "--gpus N > 1"}, {o.make_db, "--make-db"}}))
                return stop(std::string("--iterations cannot be combined with ") + with + "\n");
            if (o.topk.set && (!o.topk.ok || o.topk.i > 4096))
                return stop("--iterations reports the --topk K most significant subjects, K an integer in 1..4096\n");
            if (o.inclusion_evalue.set && !o.inclusion_evalue.ok) return stop("--inclusion-evalue must be a number > 0\n");
            if (o.max_evalue.set && !o.max_evalue.ok) return stop("--max-evalue must be a number > 0\n");
        } else if (o.inclusion_evalue.set || o.write_pssm.set) {
            return stop(std::string(o.inclusion_evalue.set ? "--inclusion-evalue" : "--write-pssm") +
                        " needs --iterations N: it belongs to the iterated search\n");
        }
        if (o.max_evalue.set && !o.iterations.set) {
            if (!o.rank.set) return stop("--max-evalue needs --rank evalue: the cutoff is applied by the ranking\n");
            if (!o.max_evalue.ok) return stop("--max-evalue must be a number > 0\n");
        }
        if (o.queries.set) {
            if (const char* with = first_of(o, {{o.query, "--query"}, {o.pssm, "--pssm"}, {o.make_db, "--make-db"},
                                                {o.gpus, "--gpus N > 1"}}))
                return stop(std::string("--queries cannot be combined with ") + with + "\n");
            const Value& k = o.hits.set ? o.hits : o.topk;
            if (o.hits.set == o.topk.set || !k.ok || k.i > 4096)
                return stop("--queries needs --hits K or --topk K, K an integer in 1..4096\n");
        }
        if (o.hits.set) {
            if (!o.hits.ok) return stop("--hits must be an integer in 1..4096\n");
            if (const char* with = first_of(o, {{o.pssm, "--pssm"}, {o.topk, "--topk"}, {o.gpus, "--gpus N > 1"},
                                                {o.make_db, "--make-db"}}))
                return stop(std::string("--hits cannot be combined with ") + with + "\n");
        }
        if (o.make_db.set && o.db.set) {
            Verdict v;
            v.what = Verdict::MAKE_DB;
            return v;
        }
    }
    // the reference: a missing required option prints the description and
    // exits 1 (main.cpp:38-41), --help likewise (main.cpp:33-36)
    if (o.query.set + o.pssm.set + o.queries.set != 1 || !o.db.set || o.help)
        return stop(o.query.set && o.pssm.set ? "--pssm takes the place of --query: give one of the two\n" : "", true);
    if (o.pssm.set && o.matrix.set)
        return stop("--pssm carries its own scores: --matrix cannot be combined with it\n");
    if (o.pssm.set && o.gpus.set && o.gpus.i != 1)
        return stop("--pssm scans on one GPU: --gpus cannot be combined with it\n");
    if (o.gpus.set && o.gpus.i < 1) return stop("", true);
    Verdict late;
    if (o.gap_open.set && !o.gap_open.ok) late = stop("--gap-open must be an integer in 1..1000\n");
    else if (o.gap_extend.set && !o.gap_extend.ok) late = stop("--gap-extend must be an integer in 1..1000\n");
    else if (o.topk.set && !o.topk.ok) late = stop("--topk must be a positive integer\n");
    late.after_matrix = late.what == Verdict::STOP && o.matrix.set;
    return late;
}

}  // namespace swcli
