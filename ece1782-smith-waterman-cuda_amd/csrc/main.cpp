// main.cpp — the FASTA scan CLI, a drop-in for the reference's bin/main
// (src/main.cpp:19-74) without boost: same flags (--help, --query, --db,
// "--opt value" or "--opt=value"), same output (the query echo, one
// "id:score" line per subject in the solver's order, the METRICS block with
// the reference's GCUPS formula: 1e-9 * |query| * sum(padded subject
// lengths) / wall seconds, wall time from program start, parsing included,
// main.cpp:20,62-72).
//
// Extra, optional: --metrics-json prints one JSON line after the METRICS
// block with the wall-clock split (FASTA parse, flatten + encode, upload =
// pack + H2D, scan); --gpus N shards the database over N GPUs (sw_group:
// residue-balanced shards, one host thread per device; same output).
// Binary databases: --make-db OUT with --db FASTA
// writes OUT (sw_db_save) and exits; --db X.swdb scans such a file with the
// same output (same ids, same order) as the FASTA it came from, without
// parsing FASTA.
// Scoring (the reference hard-wires BLOSUM50 and a linear gap of 2,
// SWSolver.cu:7-8,54-81): --matrix blosum50|blosum62|FILE, --gap-open G,
// --gap-extend E (a k-residue gap costs G + (k-1) E; E defaults to G, i.e.
// linear, G to the reference's 2).  --topk K prints only the K best subjects
// (score descending, record id ascending), ranked on the device.  Without
// these flags the output is the reference's, byte for byte.
// Profile queries: --pssm FILE takes the place of --query (exactly one of the
// two): a position-specific scoring matrix in the text format of
// sw_solver_ext.h, scanned under --gap-open / --gap-extend (--matrix has no
// meaning then and is an error).  The file and the flags are checked before
// any GPU is touched.  Output: "Input profile: N positions", the id:score
// lines, and the METRICS block with N as the query length.
// Hit table: --hits K (1..4096) prints, in place of the id:score lines, one
// tab-separated row per hit in rank order (sw_hit, sw_amd.h):
//   id score q_begin q_end s_begin s_end s_len length identities positives gap_opens gaps
// under the scoring flags, on one GPU; it cannot be combined with --pssm,
// --topk or --gpus N > 1, and is checked before any file is read.
// E-values and bit scores: --evalue, valid only with --hits (with or without
// --queries; checked before any file is read), appends two columns to every
// row, evalue (%.3g) and bits (%.1f), from the scan's own calibration
// (sw_scan_hits_sig, sw_amd.h), and prints one line per query before its rows:
//   # calibration a c sigma n_fit n_clipped status
// A calibration that clipped or is degenerate also warns on stderr: the
// scoring has no local-alignment statistic, or the database is too uniform,
// and the two columns mean nothing.  Without --evalue the output is unchanged.
// Ranking by E-value: --rank evalue, valid only with --hits K --evalue (with
// --query or --queries), prints the K most significant subjects in E-value
// order (sw_scan_hits_ranked, sw_amd.h) instead of the K best raw scores;
// --max-evalue X (X > 0), valid only with --rank evalue, keeps only subjects
// with E <= X.  Both are checked before any file is read.  The rows are the
// same 14 columns, and one more line follows a query's calibration line:
//   # significant <subjects that pass the cutoff> shown <rows>
// Without the two flags the output is unchanged.
// Batches of queries: --queries FILE takes the place of --query: a FASTA file
// of several records (sw_solver_read_queries), searched in one call of the
// library (sw_scan_batch_hits / sw_scan_batch_topk) against a FASTA or a
// .swdb database.  It needs --hits K or --topk K (1..4096) and cannot be
// combined with --query, --pssm, --make-db or --gpus N > 1 (checked before
// any file is read).  Output: "Input queries: N sequences, M residues"; per
// query in file order a line "# query <index from 0> <name> <length>" and
// its hit-table rows (--hits) or id:score lines (--topk); the METRICS block
// with M as the query length, so its GCUPS count every query's cells.
#include <sys/time.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "FASTAParsers.h"
#include "SWSolver.h"
#include "sw_amd.h"
#include "sw_solver_ext.h"

namespace {

double now_s() {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return static_cast<double>(tv.tv_usec) / 1000000 + tv.tv_sec;
}

void usage() {
    std::cout << "Smith-Waterman MI355X Usage:\n"
              << "  --help                Display this help message\n"
              << "  --query arg           Path to query file (required, or --pssm)\n"
              << "  --pssm arg            Path to a PSSM text file, in the place of --query\n"
              << "  --queries arg         Path to a multi-record FASTA file of queries, in the place of --query;\n"
              << "                        needs --hits K or --topk K (1..4096): one block of output per query\n"
              << "  --db arg              Path to database file (required; FASTA, or a .swdb file)\n"
              << "  --make-db arg         Write the FASTA --db as a binary .swdb database and exit\n"
              << "  --gpus arg            Shard the FASTA database over this many GPUs (default 1)\n"
              << "  --matrix arg          blosum50 (default, the reference's), blosum62, or a matrix file\n"
              << "  --gap-open arg        Cost of a gap's first residue (default 2)\n"
              << "  --gap-extend arg      Cost of each further gap residue (default: --gap-open, linear)\n"
              << "  --topk arg            Print only the arg best subjects (score desc, id asc)\n"
              << "  --hits arg            Print the arg best subjects (1..4096) as a hit table: id score q_begin\n"
              << "                        q_end s_begin s_end s_len length identities positives gap_opens gaps\n"
              << "  --evalue              With --hits: append evalue and bits to each row (calibrated on the\n"
              << "                        scan's own scores) and print a '# calibration' line per query\n"
              << "  --rank arg            evalue: with --hits K --evalue, rank by E-value instead of raw score and\n"
              << "                        print a '# significant N shown M' line per query\n"
              << "  --max-evalue arg      With --rank evalue: only subjects with an E-value of at most arg (> 0)\n";
}

// a whole-string integer in [lo, hi]
bool parse_int(const std::string& s, long lo, long hi, int* out) {
    char* end = nullptr;
    const long v = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || *end != '\0' || v < lo || v > hi) return false;
    *out = static_cast<int>(v);
    return true;
}

}  // namespace

int main(int argc, char* argv[]) {
    const double time_start = now_s();

    std::map<std::string, std::string> opt;
    bool help = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--help") { help = true; continue; }
        if (a.rfind("--", 0) != 0) { usage(); return 1; }
        std::string key = a.substr(2), val;
        const size_t eq = key.find('=');
        if (eq != std::string::npos) {
            val = key.substr(eq + 1);
            key = key.substr(0, eq);
        } else if (key != "metrics-json" && key != "evalue") {
            if (i + 1 >= argc) { usage(); return 1; }
            val = argv[++i];
        }
        if (key != "query" && key != "db" && key != "metrics-json" && key != "make-db" && key != "gpus" &&
            key != "matrix" && key != "gap-open" && key != "gap-extend" && key != "topk" && key != "pssm" && key != "hits" &&
            key != "queries" && key != "evalue" && key != "rank" && key != "max-evalue") {
            std::cerr << "unrecognised option '--" << key << "'\n";
            return 1;
        }
        opt[key] = val;
    }
    const bool evalue = opt.count("evalue") != 0;
    if (evalue && !opt.count("hits") && !help) {  // checked before any file is read
        std::cerr << "--evalue needs --hits K: it adds columns to the hit table\n";
        return 1;
    }
    const bool ranked = opt.count("rank") != 0;
    double max_evalue = HUGE_VAL;  // no cutoff
    if (ranked && !help) {  // checked before any file is read
        if (opt["rank"] != "evalue") {
            std::cerr << "--rank takes one value: evalue\n";
            return 1;
        }
        if (!evalue || !opt.count("hits")) {
            std::cerr << "--rank evalue needs --hits K --evalue: it orders the hit table by its evalue column\n";
            return 1;
        }
    }
    if (opt.count("max-evalue") && !help) {
        if (!ranked) {
            std::cerr << "--max-evalue needs --rank evalue: the cutoff is applied by the ranking\n";
            return 1;
        }
        char* end = nullptr;
        max_evalue = std::strtod(opt["max-evalue"].c_str(), &end);
        if (opt["max-evalue"].empty() || *end != '\0' || !(max_evalue > 0)) {
            std::cerr << "--max-evalue must be a number > 0\n";
            return 1;
        }
    }
    const bool use_queries = opt.count("queries") != 0;
    if (use_queries && !help) {  // checked before any file is read
        const char* with = opt.count("query") ? "--query" : opt.count("pssm") ? "--pssm" : nullptr;
        if (!with && opt.count("make-db")) with = "--make-db";
        if (!with && opt.count("gpus") && std::atoi(opt["gpus"].c_str()) != 1) with = "--gpus N > 1";
        if (with) {
            std::cerr << "--queries cannot be combined with " << with << "\n";
            return 1;
        }
        int k = 0;
        if (opt.count("hits") + opt.count("topk") != 1 ||
            !parse_int(opt.count("hits") ? opt["hits"] : opt["topk"], 1, 4096, &k)) {
            std::cerr << "--queries needs --hits K or --topk K, K an integer in 1..4096\n";
            return 1;
        }
    }
    int hits = 0;
    if (opt.count("hits") && !help) {  // checked before any file is read
        if (!parse_int(opt["hits"], 1, 4096, &hits)) {
            std::cerr << "--hits must be an integer in 1..4096\n";
            return 1;
        }
        const char* with = opt.count("pssm") ? "--pssm" : opt.count("topk") ? "--topk" : nullptr;
        if (!with && opt.count("gpus") && std::atoi(opt["gpus"].c_str()) != 1) with = "--gpus N > 1";
        if (!with && opt.count("make-db")) with = "--make-db";
        if (with) {
            std::cerr << "--hits cannot be combined with " << with << "\n";
            return 1;
        }
    }
    // reference: a missing required option prints the description and exits 1
    // (main.cpp:38-41), --help likewise (main.cpp:33-36)
    if (opt.count("make-db") && opt.count("db") && !help) {
        FASTADatabase fdb(opt["db"]);
        try {
            sw_save_fasta_db(fdb, opt["make-db"]);
        } catch (const std::exception& e) {
            std::cerr << e.what() << "\n";
            return 1;
        }
        cout << "Wrote " << opt["make-db"] << ": " << fdb.numSubjects << " subjects, " << fdb.subjectLengthSum
             << " padded residues." << endl;
        return 0;
    }
    const bool use_pssm = opt.count("pssm") != 0;
    if (opt.count("query") + opt.count("pssm") + opt.count("queries") != 1 || !opt.count("db") || help || argc <= 1) {
        if (opt.count("query") && use_pssm) std::cerr << "--pssm takes the place of --query: give one of the two\n";
        usage();
        return 1;
    }
    if (use_pssm && opt.count("matrix")) {
        std::cerr << "--pssm carries its own scores: --matrix cannot be combined with it\n";
        return 1;
    }
    if (use_pssm && opt.count("gpus") && std::atoi(opt["gpus"].c_str()) != 1) {
        std::cerr << "--pssm scans on one GPU: --gpus cannot be combined with it\n";
        return 1;
    }
    if (opt.count("gpus")) {
        const int n = std::atoi(opt["gpus"].c_str());
        if (n < 1) { usage(); return 1; }
        sw_solver_set_gpus(n);
    }
    // scoring: the reference's unless a scoring flag is given
    const bool custom = opt.count("matrix") || opt.count("gap-open") || opt.count("gap-extend");
    int8_t mat[625];
    int gap_open = 2, gap_extend = 2, topk = 0;
    if (custom) {
        std::string err;
        if (!use_pssm && !sw_solver_read_matrix(opt.count("matrix") ? opt["matrix"] : "blosum50", mat, &err)) {
            std::cerr << "--matrix " << err << "\n";
            return 1;
        }
        if (opt.count("gap-open") && !parse_int(opt["gap-open"], 1, 1000, &gap_open)) {
            std::cerr << "--gap-open must be an integer in 1..1000\n";
            return 1;
        }
        gap_extend = gap_open;
        if (opt.count("gap-extend") && !parse_int(opt["gap-extend"], 1, 1000, &gap_extend)) {
            std::cerr << "--gap-extend must be an integer in 1..1000\n";
            return 1;
        }
        sw_solver_set_scoring(use_pssm ? nullptr : mat, gap_open, gap_extend);
    }
    if (opt.count("topk") && !parse_int(opt["topk"], 1, INT32_MAX, &topk)) {
        std::cerr << "--topk must be a positive integer\n";
        return 1;
    }
    const std::string& dbpath = opt["db"];
    const bool binary = dbpath.size() > 5 && dbpath.compare(dbpath.size() - 5, 5, ".swdb") == 0;

    std::vector<int8_t> prows;  // --pssm: [positions][25]
    if (use_pssm) {
        std::string err;
        if (!sw_solver_read_pssm(opt["pssm"], &prows, nullptr, &err)) {
            std::cerr << "--pssm " << err << "\n";
            return 1;
        }
    }
    std::vector<std::string> qnames, qseqs;  // --queries
    size_t qresidues = 0;
    if (use_queries) {
        std::string err;
        if (!sw_solver_read_queries(opt["queries"], &qnames, &qseqs, &err)) {
            std::cerr << "--queries " << err << "\n";
            return 1;
        }
        for (const std::string& s : qseqs) qresidues += s.size();
    }
    FASTAQuery query(use_pssm || use_queries ? std::string() : opt["query"], true);  // (no file: an empty buffer)
    if (use_pssm) {
        cout << "Input profile: " << prows.size() / 25 << " positions" << endl;
    } else if (use_queries) {
        cout << "Input queries: " << qseqs.size() << " sequences, " << qresidues << " residues" << endl;
    } else {
        cout << "Input buffer:";
        query.print_buffer();
        cout << endl;
    }
    // the query length of the METRICS block: the PSSM's positions, a batch's residues
    const string querySequence = use_pssm      ? string(prows.size() / 25, 'X')
                                 : use_queries ? string(qresidues, 'X')
                                               : query.get_buffer();

    vector<seqid_score> result;
    result.reserve(use_queries ? 0 : 600000);
    std::vector<sw_hit> rows;  // --hits
    std::vector<std::vector<seqid_score> > bresult;  // --queries: one block per query
    std::vector<std::vector<sw_hit> > brows;
    std::vector<sw_sig> sigs;  // --evalue: beside rows / brows
    std::vector<std::vector<sw_sig> > bsigs;
    std::vector<sw_calib> calibs;  // ... one per query
    std::vector<int64_t> npass;    // --rank evalue: per query, the subjects that pass the cutoff
    int64_t num_subjects = 0, length_sum = 0;
    double solve_s = 0, parse_s = 0;
    if (!binary) {
        const double t_parse = now_s();
        FASTADatabase db(dbpath);
        parse_s = now_s() - t_parse;
        const double t_solve = now_s();
        try {
            if (use_queries && ranked)
                brows = smith_waterman_cuda_batch_hits_ranked(qseqs, db, hits, max_evalue, &bsigs, &npass, &calibs);
            else if (ranked) {
                calibs.resize(1);
                npass.resize(1);
                rows = smith_waterman_cuda_hits_ranked(query, db, hits, max_evalue, &sigs, &npass[0], &calibs[0]);
            }
            else if (use_queries && hits && evalue) brows = smith_waterman_cuda_batch_hits_sig(qseqs, db, hits, &bsigs, &calibs);
            else if (hits && evalue) {
                calibs.resize(1);
                rows = smith_waterman_cuda_hits_sig(query, db, hits, &sigs, &calibs[0]);
            }
            else if (use_queries && hits) brows = smith_waterman_cuda_batch_hits(qseqs, db, hits);
            else if (use_queries) bresult = smith_waterman_cuda_batch_topk(qseqs, db, topk);
            else if (hits) rows = smith_waterman_cuda_hits(query, db, hits);
            else if (use_pssm) result = smith_waterman_cuda_pssm(prows, db, topk);
            else if (topk) result = smith_waterman_cuda_topk(query, db, topk);
            else smith_waterman_cuda(query, db, result);
        } catch (const std::exception& e) {
            std::cerr << e.what() << "\n";
            return 1;
        }
        solve_s = now_s() - t_solve;
        num_subjects = db.numSubjects;
        length_sum = db.subjectLengthSum;
    } else {
        // the file holds the reference's order and record ids (sw_save_fasta_db)
        auto die = [](const char* what) {
            std::cerr << what << ": " << sw_last_error() << "\n";
            return 1;
        };
        sw_handle* h = nullptr;
        const char* dev = std::getenv("SW_DEVICE");
        if (sw_create(dev ? std::atoi(dev) : 0, &h)) return die("sw_create");
        sw_db* sdb = nullptr;
        if (sw_db_load(h, dbpath.c_str(), &sdb)) return die("sw_db_load");
        sw_db_stats st;
        sw_db_get_stats(sdb, &st);
        std::vector<int64_t> lens(static_cast<size_t>(st.n_subjects));
        std::vector<int32_t> ids(static_cast<size_t>(st.n_subjects));
        sw_db_subjects(sdb, lens.data(), ids.data());
        std::string q = query.get_buffer();
        // the reference pads the query (SWSolver.cu:267-269); its pad rows
        // score 0 only under its own table (see swsolver.cpp encode_query);
        // a hit table's coordinates are those of the query as written
        while (!custom && !hits && q.size() % 8 != 0) q += "/";
        std::vector<uint8_t> qc(q.size());
        sw_encode(q.data(), static_cast<int64_t>(q.size()), qc.data());
        // BLOSUM50 (SWSolver.cu:54-81), gap 2 (:7), unless chosen
        const sw_scoring sc = {custom ? mat : nullptr, gap_open, gap_extend};
        sw_pssm* pssm = nullptr;
        if (use_pssm && sw_pssm_create(h, prows.data(), static_cast<int32_t>(prows.size() / 25), &pssm))
            return die("sw_pssm_create");
        const double t_solve = now_s();
        if (use_queries) {
            // the queries as written, concatenated (sw_scan_batch's form)
            const int32_t nq = static_cast<int32_t>(qseqs.size());
            std::vector<int64_t> qoffs(qseqs.size() + 1, 0);
            for (size_t i = 0; i < qseqs.size(); ++i) qoffs[i + 1] = qoffs[i] + static_cast<int64_t>(qseqs[i].size());
            std::vector<uint8_t> cat(qresidues);
            for (size_t i = 0; i < qseqs.size(); ++i)
                sw_encode(qseqs[i].data(), static_cast<int64_t>(qseqs[i].size()), cat.data() + qoffs[i]);
            if (hits) {
                std::vector<sw_hit> all(qseqs.size() * static_cast<size_t>(hits));
                int32_t nhits = 0;
                std::vector<sw_sig> allsig(evalue ? all.size() : 0);
                calibs.resize(evalue ? qseqs.size() : 0);
                std::vector<int32_t> qhits(qseqs.size(), 0);  // --rank evalue: a query's row count is its own
                npass.resize(ranked ? qseqs.size() : 0);
                if (ranked) {
                    if (sw_scan_batch_hits_ranked(h, sdb, cat.data(), qoffs.data(), nq, &sc, hits, max_evalue, 0, all.data(),
                                                  allsig.data(), qhits.data(), npass.data(), calibs.data()))
                        return die("sw_scan_batch_hits_ranked");
                } else if (evalue ? sw_scan_batch_hits_sig(h, sdb, cat.data(), qoffs.data(), nq, &sc, hits, all.data(),
                                                    allsig.data(), &nhits, calibs.data())
                           : sw_scan_batch_hits(h, sdb, cat.data(), qoffs.data(), nq, &sc, hits, all.data(), &nhits))
                    return die("sw_scan_batch_hits");
                for (size_t i = 0; i < qseqs.size(); ++i) {
                    if (ranked) nhits = qhits[i];
                    brows.push_back(std::vector<sw_hit>(all.begin() + static_cast<int64_t>(i) * hits,
                                                        all.begin() + static_cast<int64_t>(i) * hits + nhits));
                    if (evalue)
                        bsigs.push_back(std::vector<sw_sig>(allsig.begin() + static_cast<int64_t>(i) * hits,
                                                            allsig.begin() + static_cast<int64_t>(i) * hits + nhits));
                }
            } else {
                std::vector<int64_t> keys(qseqs.size() * static_cast<size_t>(topk));
                if (sw_scan_batch_topk(h, sdb, cat.data(), qoffs.data(), nq, &sc, topk, keys.data()))
                    return die("sw_scan_batch_topk");
                bresult.resize(qseqs.size());
                for (size_t i = 0; i < qseqs.size(); ++i)
                    for (int j = 0; j < topk; ++j) {
                        const int64_t key = keys[i * static_cast<size_t>(topk) + j];
                        if (key == INT64_MIN) break;
                        bresult[i].push_back(std::make_pair(static_cast<int>((int64_t{1} << 31) - 1 - (key & 0xffffffff)),
                                                            static_cast<int>(key >> 32)));
                    }
            }
        } else if (hits) {
            rows.resize(static_cast<size_t>(hits));
            int32_t nhits = 0;
            sigs.resize(evalue ? rows.size() : 0);
            calibs.resize(evalue ? 1 : 0);
            npass.resize(ranked ? 1 : 0);
            if (ranked) {
                if (sw_scan_hits_ranked(h, sdb, qc.data(), static_cast<int32_t>(qc.size()), &sc, hits, max_evalue,
                                        rows.data(), sigs.data(), &nhits, npass.data(), calibs.data()))
                    return die("sw_scan_hits_ranked");
            } else if (evalue ? sw_scan_hits_sig(h, sdb, qc.data(), static_cast<int32_t>(qc.size()), &sc, hits, rows.data(),
                                          sigs.data(), &nhits, calibs.data())
                       : sw_scan_hits(h, sdb, qc.data(), static_cast<int32_t>(qc.size()), &sc, hits, rows.data(), &nhits))
                return die("sw_scan_hits");
            rows.resize(static_cast<size_t>(nhits));
            sigs.resize(evalue ? rows.size() : 0);
        } else if (topk && topk <= 4096) {
            std::vector<int64_t> keys(static_cast<size_t>(topk));
            if (use_pssm ? sw_scan_pssm_topk(h, sdb, pssm, gap_open, gap_extend, topk, keys.data())
                         : sw_scan_topk(h, sdb, qc.data(), static_cast<int32_t>(qc.size()), &sc, topk, keys.data()))
                return die("sw_scan_topk");
            for (int64_t key : keys) {
                if (key == INT64_MIN) break;
                result.push_back(std::make_pair(static_cast<int>((int64_t{1} << 31) - 1 - (key & 0xffffffff)),
                                                static_cast<int>(key >> 32)));
            }
        } else {
            std::vector<int32_t> scores(static_cast<size_t>(st.max_id + 1), 0);
            if (st.n_subjects &&
                (use_pssm ? sw_scan_pssm(h, sdb, pssm, gap_open, gap_extend, scores.data())
                          : sw_scan(h, sdb, qc.data(), static_cast<int32_t>(qc.size()), &sc, scores.data())))
                return die("sw_scan");
            // the reference's report order: padded length descending, file
            // (= record id) order within a length (SWSolver.cu:309,384-390)
            std::vector<int64_t> order(static_cast<size_t>(st.n_subjects));
            for (int64_t k = 0; k < st.n_subjects; ++k) order[k] = k;
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
                const int pa = roundUp(static_cast<int>(lens[a]), TILE_SIZE), pb = roundUp(static_cast<int>(lens[b]), TILE_SIZE);
                return pa != pb ? pa > pb : ids[a] < ids[b];
            });
            for (int64_t k : order) result.push_back(std::make_pair(static_cast<int>(ids[k]), scores[ids[k]]));
            if (topk) {  // beyond the device top-K's 4096: ranked here
                const size_t kk = std::min<size_t>(result.size(), static_cast<size_t>(topk));
                std::partial_sort(result.begin(), result.begin() + kk, result.end(),
                                  [](const seqid_score& a, const seqid_score& b) {
                                      return a.second != b.second ? a.second > b.second : a.first < b.first;
                                  });
                result.resize(kk);
            }
        }
        solve_s = now_s() - t_solve;
        // the FASTA parser's padded sizes (TILE_SIZE, FASTAParsers.h): files
        // hold the subjects as written (older ones '/'-padded: the same sums)
        for (int64_t k = 0; k < st.n_subjects; ++k) length_sum += roundUp(static_cast<int>(lens[k]), TILE_SIZE);
        num_subjects = st.n_subjects;
        sw_pssm_free(pssm);
        sw_db_free(sdb);
        sw_destroy(h);
    }

    auto print_scores = [](const vector<seqid_score>& v) {
        for (vector<seqid_score>::const_iterator it = v.begin(); it != v.end(); ++it)
            cout << (*it).first << ":" << (*it).second << "\n";
    };
    // sig (nullable): the rows' significances, two more columns
    auto print_rows = [](const std::vector<sw_hit>& v, const std::vector<sw_sig>* sig) {
        for (size_t i = 0; i < v.size(); ++i) {
            const sw_hit& r = v[i];
            cout << r.id << "\t" << r.score << "\t" << r.q_begin << "\t" << r.q_end << "\t" << r.s_begin << "\t"
                 << r.s_end << "\t" << r.s_len << "\t" << r.length << "\t" << r.identities << "\t" << r.positives
                 << "\t" << r.gap_opens << "\t" << r.gaps;
            if (sig) {
                char buf[64];
                std::snprintf(buf, sizeof buf, "\t%.3g\t%.1f", (*sig)[i].evalue, (*sig)[i].bits);
                cout << buf;
            }
            cout << "\n";
        }
    };
    // --evalue: a query's calibration line, and the warning when it carries no statistic
    auto print_calib = [](const sw_calib& c, size_t query_index) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "# calibration %.6g %.6g %.6g %lld %lld %d\n", c.a, c.c, c.sigma,
                      static_cast<long long>(c.n_fit), static_cast<long long>(c.n_clipped), c.status);
        cout << buf;
        if (c.status & SW_CALIB_CLIPPED)
            std::cerr << "warning: query " << query_index << ": " << c.n_clipped << " of " << c.n_db
                      << " scores reach the calibration's clip column (511): under this scoring scores grow with"
                         " length and the evalue and bits columns mean nothing\n";
        if (c.status & SW_CALIB_DEGENERATE)
            std::cerr << "warning: query " << query_index
                      << ": the calibration is degenerate (too few or too uniform scores): every evalue is the"
                         " database's size\n";
    };
    // --rank evalue: how many subjects passed the cutoff, and how many of them are shown
    auto print_significant = [&](size_t i, size_t shown) {
        if (i < npass.size()) cout << "# significant " << npass[i] << " shown " << shown << "\n";
    };
    print_scores(result);
    if (evalue && !use_queries && !calibs.empty()) print_calib(calibs[0], 0);
    if (!use_queries) print_significant(0, rows.size());
    print_rows(rows, evalue && !use_queries ? &sigs : nullptr);
    // --queries: a block per query, in file order (index from 0; "-" for a header without a name)
    for (size_t i = 0; i < qseqs.size(); ++i) {
        cout << "# query " << i << " " << (qnames[i].empty() ? "-" : qnames[i]) << " " << qseqs[i].size() << "\n";
        if (evalue && i < calibs.size()) print_calib(calibs[i], i);
        if (i < brows.size()) print_significant(i, brows[i].size());
        if (i < brows.size()) print_rows(brows[i], evalue && i < bsigs.size() ? &bsigs[i] : nullptr);
        if (i < bresult.size()) print_scores(bresult[i]);
    }

    const double seconds_elapsed = now_s() - time_start;
    cout << std::string(80, '=') << endl;
    cout << "METRICS:" << endl;
    cout << "Query length: " << querySequence.length() << " chars." << endl;
    cout << "Num subjects: " << num_subjects << endl;
    cout << "Sum of DB length: " << length_sum << " chars." << endl;
    cout << "Time elapsed: " << seconds_elapsed << " seconds." << endl;
    cout << "Performance: " << 1E-9 * (querySequence.length() * static_cast<double>(length_sum)) / seconds_elapsed
         << " GCUPS." << endl;
    if (opt.count("metrics-json")) {
        const sw_solver_timing t = sw_solver_last_timing();
        cout << "{\"query_len\": " << querySequence.length() << ", \"subjects\": " << num_subjects
             << ", \"padded_residues\": " << length_sum << ", \"wall_s\": " << seconds_elapsed
             << ", \"parse_s\": " << parse_s << ", \"solve_s\": " << solve_s << ", \"flatten_s\": " << t.flatten_s
             << ", \"init_s\": " << t.init_s << ", \"upload_s\": " << t.upload_s << ", \"scan_s\": " << t.scan_s
             << ", \"gpus\": " << t.gpus
             << "}" << endl;
    }
    return 0;
}
