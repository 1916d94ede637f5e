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
// Iterated profile search: --iterations N with --query (sw_search_iter,
// sw_amd.h): up to N rounds, each scanning the current profile, including the
// subjects with E <= --inclusion-evalue X (default 1e-3) and rebuilding the
// profile from their alignments.  It cannot be combined with --pssm,
// --queries, --hits, --gpus N > 1 or --make-db; --topk K (1..4096, default
// 500) and --max-evalue X bound the report; all checked before any file is
// read.  Output after the query echo: per round
//   # iteration <t> included <n> added <a> dropped <d>
// then "# converged" or "# stopped after <N>", then per reported subject, in
// E-value order, a tab-separated row: id score evalue bits.  --write-pssm FILE
// writes the last round's profile in --pssm's format.
//
// Five steps: parse and validate the flags (sw_cli.h: pure, no file read),
// read the inputs, search (sw_solver_search: one path for a FASTA and a .swdb
// database), print.
#include <sys/time.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "FASTAParsers.h"
#include "SWSolver.h"
#include "sw_amd.h"
#include "sw_cli.h"
#include "sw_solver_ext.h"

namespace {

double now_s() {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return static_cast<double>(tv.tv_usec) / 1000000 + tv.tv_sec;
}

int stop(const swcli::Verdict& v) {
    std::cerr << v.err;
    if (v.usage) std::cout << swcli::usage_text();
    return v.code;
}

int make_db(const swcli::Options& o) {
    FASTADatabase fdb(o.db.text);
    try {
        sw_save_fasta_db(fdb, o.make_db.text);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    cout << "Wrote " << o.make_db.text << ": " << fdb.numSubjects << " subjects, " << fdb.subjectLengthSum
         << " padded residues." << endl;
    return 0;
}

void print_scores(const vector<seqid_score>& v) {
    for (const seqid_score& s : v) cout << s.first << ":" << s.second << "\n";
}

// sig (nullable): the rows' significances, two more columns
void print_rows(const std::vector<sw_hit>& v, const std::vector<sw_sig>* sig) {
    for (size_t i = 0; i < v.size(); ++i) {
        const sw_hit& r = v[i];
        cout << r.id << "\t" << r.score << "\t" << r.q_begin << "\t" << r.q_end << "\t" << r.s_begin << "\t" << r.s_end
             << "\t" << r.s_len << "\t" << r.length << "\t" << r.identities << "\t" << r.positives << "\t"
             << r.gap_opens << "\t" << r.gaps;
        if (sig) {
            char buf[64];
            std::snprintf(buf, sizeof buf, "\t%.3g\t%.1f", (*sig)[i].evalue, (*sig)[i].bits);
            cout << buf;
        }
        cout << "\n";
    }
}

// --evalue: a query's calibration line, and the warning when it carries no statistic
void print_calib(const sw_calib& c, size_t query_index) {
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
}

// --iterations: the rounds' trace, how the loop ended, and the report
void print_iterations(const sw_search_result& r, long rounds) {
    for (size_t t = 0; t < r.rounds.size(); ++t)
        cout << "# iteration " << t + 1 << " included " << r.rounds[t].included << " added " << r.rounds[t].added
             << " dropped " << r.rounds[t].dropped << "\n";
    if (r.converged) cout << "# converged\n";
    else cout << "# stopped after " << rounds << "\n";
    for (size_t i = 0; i < r.scores[0].size(); ++i) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "%d\t%d\t%.3g\t%.1f\n", r.scores[0][i].first, r.scores[0][i].second,
                      r.iter_sigs[i].evalue, r.iter_sigs[i].bits);
        cout << buf;
    }
}

}  // namespace

int main(int argc, char* argv[]) {
    const double time_start = now_s();

    swcli::Options o;
    swcli::Verdict v = swcli::parse(argc, argv, &o);
    if (v.what == swcli::Verdict::PROCEED) v = swcli::validate(o);
    if (v.what == swcli::Verdict::MAKE_DB) return make_db(o);
    // the one check that reads a file amid the flags': a --matrix file's own
    // error goes before those of the gap and top-K values
    if (v.what == swcli::Verdict::STOP && !v.after_matrix) return stop(v);
    int8_t mat[625];
    if (o.custom() && !o.pssm.set) {
        std::string err;
        if (!sw_solver_read_matrix(o.matrix.set ? o.matrix.text : "blosum50", mat, &err)) {
            std::cerr << "--matrix " << err << "\n";
            return 1;
        }
    }
    if (v.what == swcli::Verdict::STOP) return stop(v);
    if (o.gpus.set) sw_solver_set_gpus(static_cast<int>(o.gpus.i));
    // scoring: the reference's unless a scoring flag is given
    if (o.custom()) sw_solver_set_scoring(o.pssm.set ? nullptr : mat, o.gap_open_cost(), o.gap_extend_cost());

    // the inputs; the query length of the METRICS block is the PSSM's positions or a batch's residues
    std::vector<int8_t> prows;  // --pssm: [positions][25]
    std::vector<std::string> qnames, qseqs;  // --queries
    std::string err;
    if (o.pssm.set && !sw_solver_read_pssm(o.pssm.text, &prows, nullptr, &err)) {
        std::cerr << "--pssm " << err << "\n";
        return 1;
    }
    if (o.queries.set && !sw_solver_read_queries(o.queries.text, &qnames, &qseqs, &err)) {
        std::cerr << "--queries " << err << "\n";
        return 1;
    }
    FASTAQuery query(o.query.set ? o.query.text : std::string(), true);  // (no file: an empty buffer)
    const std::string qbuf = query.get_buffer();
    size_t query_len = o.pssm.set ? prows.size() / 25 : qbuf.size();
    for (const std::string& s : qseqs) query_len += s.size();
    if (o.pssm.set) {
        cout << "Input profile: " << query_len << " positions" << endl;
    } else if (o.queries.set) {
        cout << "Input queries: " << qseqs.size() << " sequences, " << query_len << " residues" << endl;
    } else {
        cout << "Input buffer:";
        query.print_buffer();
        cout << endl;
    }

    sw_search_request rq = {};
    if (o.pssm.set) rq.pssm = &prows;
    else if (o.queries.set) rq.queries = &qseqs;
    else rq.query = &qbuf;
    rq.mode = o.hits.set ? sw_search_request::HITS : o.topk.set ? sw_search_request::TOPK : sw_search_request::SCORES;
    rq.k = static_cast<int>(o.hits.set ? o.hits.i : o.topk.set ? o.topk.i : 0);
    if (o.iterations.set) {
        rq.mode = sw_search_request::TOPK;
        rq.k = o.iter_topk();
        rq.iterations = static_cast<int>(o.iterations.i);
        rq.inclusion_evalue = o.iter_inclusion();
    }
    rq.evalue = o.evalue.set;
    rq.ranked = o.ranked();
    rq.max_evalue = o.max_evalue.set ? o.max_evalue.d : HUGE_VAL;  // no cutoff
    sw_search_result r;
    try {
        r = sw_solver_search(o.db.text, rq);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 1;
    }

    if (o.iterations.set) {
        print_iterations(r, o.iterations.i);
        if (o.write_pssm.set && !sw_solver_write_pssm(o.write_pssm.text, r.final_pssm, r.final_consensus, &err)) {
            std::cerr << "--write-pssm " << err << "\n";
            return 1;
        }
        r.scores.clear();  // (printed above, with their significances)
    }

    // per query (--queries: a block each, in file order; index from 0, "-" for a header without a name)
    for (size_t i = 0; i < (o.queries.set ? qseqs.size() : 1); ++i) {
        if (o.queries.set)
            cout << "# query " << i << " " << (qnames[i].empty() ? "-" : qnames[i]) << " " << qseqs[i].size() << "\n";
        if (i < r.calibs.size()) print_calib(r.calibs[i], i);
        // --rank evalue: how many subjects passed the cutoff, and how many of them are shown
        if (i < r.n_pass.size()) cout << "# significant " << r.n_pass[i] << " shown " << r.rows[i].size() << "\n";
        if (i < r.rows.size()) print_rows(r.rows[i], i < r.sigs.size() ? &r.sigs[i] : nullptr);
        if (i < r.scores.size()) print_scores(r.scores[i]);
    }

    const double seconds_elapsed = now_s() - time_start;
    cout << std::string(80, '=') << endl;
    cout << "METRICS:" << endl;
    cout << "Query length: " << query_len << " chars." << endl;
    cout << "Num subjects: " << r.num_subjects << endl;
    cout << "Sum of DB length: " << r.padded_residues << " chars." << endl;
    cout << "Time elapsed: " << seconds_elapsed << " seconds." << endl;
    cout << "Performance: " << 1E-9 * (query_len * static_cast<double>(r.padded_residues)) / seconds_elapsed
         << " GCUPS." << endl;
    if (o.metrics_json.set) {
        const sw_solver_timing t = sw_solver_last_timing();
        cout << "{\"query_len\": " << query_len << ", \"subjects\": " << r.num_subjects
             << ", \"padded_residues\": " << r.padded_residues << ", \"wall_s\": " << seconds_elapsed
             << ", \"parse_s\": " << r.parse_s << ", \"solve_s\": " << r.solve_s << ", \"flatten_s\": " << t.flatten_s
             << ", \"init_s\": " << t.init_s << ", \"upload_s\": " << t.upload_s << ", \"scan_s\": " << t.scan_s
             << ", \"gpus\": " << t.gpus
             << "}" << endl;
    }
    return 0;
}
