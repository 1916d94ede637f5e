// swsolver.cpp — the reference's C++ solver entry points over the C ABI.
//
//   smith_waterman_cuda       (reference SWSolver.h:9,  SWSolver.cu:266-404)
//   smith_waterman_cuda_char  (reference SWSolver_char.h:9, SWSolver_char.cu:193-280)
//
// One process-wide handle on device $SW_DEVICE (default 0), created on first
// use.  With $SW_GPUS = N > 1 (or sw_solver_set_gpus, `main --gpus N`) the
// database is sharded over devices 0..N-1 (or the list in $SW_DEVICES) by a
// process-wide sw_group (sw_amd.h: residue-balanced shards, one host thread
// per device); the result vector is identical to the one-GPU path.  The
// database is flattened in the order the reference reports results
// (descending padded length, file order within a length: SWSolver.cu:309,
// 384-390), uploaded, scanned and freed per call, like the reference does
// (it re-packs per call too, SWSolver.cu:301-371).  Flattening + encoding
// runs on the host's cores; sw_solver_last_timing() splits the call into
// flatten / device start-up (first call only) / upload (pack + H2D) / scan.
//
// Scoring: the reference's (BLOSUM50 of SWSolver.cu:54-81, linear gap 2 of
// SWSolver.cu:7) unless sw_solver_set_scoring chose another matrix / gap
// model (`main --matrix --gap-open --gap-extend`); smith_waterman_cuda_topk
// returns only the k best subjects, ranked on the device (`main --topk`).
//
// Every entry point, and `main` through sw_solver_search, is one request to
// search() below: the subjects (a FASTADatabase flattened, or a .swdb file
// loaded), the timed stages, and the one library call the request names.
#include <sys/time.h>

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "SWSolver.h"
#include "SWSolver_char.h"
#include "sw_abi_ptr.h"
#include "sw_amd.h"
#include "sw_solver_ext.h"

namespace {

std::mutex g_mu;
// process-wide, and alive until the process ends: torn down from a static
// destructor they would race the HIP runtime's own
sw_handle_ptr& g_handle = *new sw_handle_ptr;
sw_group_ptr& g_group = *new sw_group_ptr;
int g_gpus = 0;  // 0: $SW_GPUS or 1
sw_solver_timing g_timing = {};
// the scoring of smith_waterman_cuda[_topk]; custom = false: the reference's
struct SolverScoring {
    bool custom = false;
    bool has_matrix = false;
    int8_t mat[625] = {};
    int go = 2, ge = 2;
} g_sc;

void check(int rc, const char* what) {
    if (rc != SW_OK) throw std::runtime_error(std::string(what) + ": " + sw_last_error());
}

double now_s() {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return static_cast<double>(tv.tv_usec) / 1000000 + tv.tv_sec;
}

// The wall time of a scope, added to one field of g_timing.
struct Stage {
    double& field;
    const double t0 = now_s();
    explicit Stage(double& f) : field(f) {}
    ~Stage() { field += now_s() - t0; }
};

int gpus() {
    if (g_gpus > 0) return g_gpus;
    const char* e = std::getenv("SW_GPUS");
    const int n = e ? std::atoi(e) : 1;
    return n > 0 ? n : 1;
}

sw_handle* handle() {
    if (!g_handle) {
        const char* dev = std::getenv("SW_DEVICE");
        sw_handle* h = nullptr;
        check(sw_create(dev ? std::atoi(dev) : 0, &h), "sw_create");
        g_handle.reset(h);
    }
    return g_handle.get();
}

// The group over the first gpus() devices ($SW_DEVICES="a,b,..." overrides
// the list, e.g. "0,0" to run the sharded path on a one-GPU machine).
sw_group* group() {
    const int n = gpus();
    if (g_group) return g_group.get();
    std::vector<int32_t> devs;
    if (const char* e = std::getenv("SW_DEVICES")) {
        std::string s(e);
        size_t at = 0;
        while (at <= s.size() && static_cast<int>(devs.size()) < n) {
            const size_t c = s.find(',', at);
            devs.push_back(std::atoi(s.substr(at, c == std::string::npos ? std::string::npos : c - at).c_str()));
            if (c == std::string::npos) break;
            at = c + 1;
        }
    }
    for (int d = static_cast<int>(devs.size()); d < n; ++d) devs.push_back(d);
    sw_group* g = nullptr;
    check(sw_group_create(devs.data(), n, &g), "sw_group_create");
    g_group.reset(g);
    return g;
}

// The subjects of one search: their record ids in the database's own order,
// what the report needs, and the database itself — loaded from a file, or
// uploaded by search() from the flattened residues.
struct Subjects {
    std::vector<uint8_t> residues;  // a FASTA's, encoded; empty for a file
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> ids;    // record id of each subject
    std::vector<int64_t> order;  // the plain scan's report order: indices into ids
    sw_db_ptr db;
    sw_gdb_ptr gdb;  // ... or sharded over the group
    bool from_file = false;
    int64_t max_id = -1;                        // a file's scores are indexed by record id
    int64_t num_subjects = 0, padded_sum = 0;  // METRICS: the FASTA parser's counts (TILE_SIZE padding)

    Subjects(FASTADatabase& fdb, bool strip_pad);
    explicit Subjects(const std::string& path);
    int64_t n() const { return static_cast<int64_t>(ids.size()); }
    int64_t score_slot(int64_t k) const { return from_file ? ids[static_cast<size_t>(k)] : k; }
};

// Flatten in the reference's reporting order; the encoding (SWSolver.cu:91-
// 120) of the concatenated residues is split over the host's cores.
// strip_pad: without the parser's '/' padding (FASTAParsers.h pads every
// subject to a multiple of TILE_SIZE; '/' encodes as '*'): the subjects as
// written.  Under the reference's BLOSUM50 the pad scores 0 and changes no
// score, so it is kept there; other scorings (BLOSUM62: '*' +1 against '*')
// and the binary database files get the subjects as written.
Subjects::Subjects(FASTADatabase& fdb, bool strip_pad) {
    Stage flatten(g_timing.flatten_s);
    std::vector<const subject_sequence*> subj;
    subj.reserve(fdb.numSubjects > 0 ? static_cast<size_t>(fdb.numSubjects) : 0);
    for (auto it = fdb.parsedDB.rbegin(); it != fdb.parsedDB.rend(); ++it)
        for (const subject_sequence& s : it->second) subj.push_back(&s);
    const size_t n = subj.size();
    offsets.resize(n + 1);
    ids.resize(n);
    auto len_of = [&](size_t k) {
        const std::string& s = subj[k]->sequence;
        size_t m = s.size();
        while (strip_pad && m > 0 && s[m - 1] == '/') --m;
        return m;
    };
    for (size_t k = 0; k < n; ++k) {
        offsets[k + 1] = offsets[k] + static_cast<int64_t>(len_of(k));
        ids[k] = subj[k]->id;
    }
    residues.resize(static_cast<size_t>(offsets[n]));
    uint8_t probe;
    check(sw_encode("A", 1, &probe), "sw_encode");  // the code table exists before the threads start
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < 4096) nt = 1;
    std::vector<std::thread> th;
    std::vector<int> rc(nt, SW_OK);
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (size_t k = t; k < n; k += nt) {
                const std::string& s = subj[k]->sequence;
                const int r = sw_encode(s.data(), offsets[k + 1] - offsets[k], residues.data() + offsets[k]);
                if (r) rc[t] = r;
            }
        });
    for (auto& x : th) x.join();
    for (int r : rc) check(r, "sw_encode");
    order.resize(n);
    std::iota(order.begin(), order.end(), int64_t{0});
    num_subjects = fdb.numSubjects;
    padded_sum = fdb.subjectLengthSum;
}

// A .swdb file holds the flattened order, the record ids and the subjects as
// written (sw_save_fasta_db).  The report order is the reference's: padded
// length descending, file (= record id) order within a length
// (SWSolver.cu:309,384-390); the padded sizes are the FASTA parser's
// (TILE_SIZE; older files hold '/'-padded subjects: the same sums).
Subjects::Subjects(const std::string& path) : from_file(true) {
    sw_handle* h = nullptr;
    {
        Stage init(g_timing.init_s);
        h = handle();
    }
    {
        Stage upload(g_timing.upload_s);
        sw_db* loaded = nullptr;
        check(sw_db_load(h, path.c_str(), &loaded), "sw_db_load");
        db.reset(loaded);
    }
    sw_db_stats st;
    check(sw_db_get_stats(db.get(), &st), "sw_db_get_stats");
    std::vector<int64_t> lens(static_cast<size_t>(st.n_subjects));
    ids.resize(lens.size());
    check(sw_db_subjects(db.get(), lens.data(), ids.data()), "sw_db_subjects");
    auto padded = [&](int64_t k) { return roundUp(static_cast<int>(lens[static_cast<size_t>(k)]), TILE_SIZE); };
    order.resize(lens.size());
    std::iota(order.begin(), order.end(), int64_t{0});
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return padded(a) != padded(b) ? padded(a) > padded(b) : ids[a] < ids[b];
    });
    for (int64_t k = 0; k < st.n_subjects; ++k) padded_sum += padded(k);
    num_subjects = st.n_subjects;
    max_id = st.max_id;
}

std::vector<uint8_t> encode(const std::string& s) {
    std::vector<uint8_t> codes(s.size());
    check(sw_encode(s.data(), static_cast<int64_t>(s.size()), codes.data()), "sw_encode");
    return codes;
}

// The queries as written, concatenated (sw_scan_batch's form).
void concat_queries(const std::vector<std::string>& seqs, std::vector<uint8_t>* codes, std::vector<int64_t>* offs) {
    offs->assign(seqs.size() + 1, 0);
    for (size_t q = 0; q < seqs.size(); ++q) (*offs)[q + 1] = (*offs)[q] + static_cast<int64_t>(seqs[q].size());
    codes->resize(static_cast<size_t>(offs->back()));
    for (size_t q = 0; q < seqs.size(); ++q)
        check(sw_encode(seqs[q].data(), static_cast<int64_t>(seqs[q].size()), codes->data() + (*offs)[q]), "sw_encode");
}

// A device top-K key (sw_amd.h sw_scan_topk) as (record id, score); the keys
// of one query end at k or at the first INT64_MIN (fewer subjects than k).
seqid_score decode_key(int64_t key) {
    return std::make_pair(static_cast<int>((int64_t{1} << 31) - 1 - (key & 0xffffffff)), static_cast<int>(key >> 32));
}

// Score descending, record id ascending: the device top-K's order, for a k
// beyond its 4096 or record ids it cannot carry (a headerless file's -1).
void rank_on_host(std::vector<seqid_score>* v, int k) {
    const size_t kk = std::min<size_t>(v->size(), static_cast<size_t>(k));
    std::partial_sort(v->begin(), v->begin() + kk, v->end(), [](const seqid_score& a, const seqid_score& b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    v->resize(kk);
}

// Query q's n rows of a table that holds k per query.
template <class T>
std::vector<T> rows_of(const std::vector<T>& all, size_t q, int k, int32_t n) {
    const auto at = all.begin() + static_cast<int64_t>(q) * k;
    return std::vector<T>(at, at + n);
}

// The two departures of smith_waterman_cuda_char from a plain scan: the
// subjects keep the parser's padding under any scoring, and with
// SW_CHAR_COMPAT=1 the scoring is the _char path's own table.
enum class CharPath { NO, ORDER, TABLE };

// The library entry point a request goes to, as the error texts name it (a
// loaded file's have never said _pssm or _sig).
std::string entry_name(const sw_search_request& rq, bool from_file, bool group, bool all_scores) {
    std::string name = group ? "sw_group" : "sw_scan";
    if (rq.queries) name += "_batch";
    if (rq.pssm && !from_file) name += "_pssm";
    if (all_scores) name += group ? "_scan" : "";
    else name += rq.mode == sw_search_request::HITS ? "_hits" : "_topk";
    if (rq.ranked) name += "_ranked";
    else if (rq.evalue && !from_file) name += "_sig";
    return name;
}

// One search: exactly one of fdb / file names the subjects.
sw_search_result search(FASTADatabase* fdb, const std::string& file, const sw_search_request& rq,
                        CharPath cp = CharPath::NO) {
    const bool batch = rq.queries != nullptr, hits = rq.mode == sw_search_request::HITS;
    const bool iter = rq.iterations > 0;
    const int k = rq.k;
    if (iter && (!rq.query || rq.mode != sw_search_request::TOPK || k < 1 || k > 4096 || rq.evalue || rq.ranked ||
                 !(rq.inclusion_evalue > 0) || !(rq.max_evalue > 0)))
        throw std::invalid_argument("an iterated search takes one query, reports its 1 <= k <= 4096 most significant "
                                    "subjects and needs E-value bounds > 0");
    if (!rq.query + !rq.queries + !rq.pssm != 2)
        throw std::invalid_argument("a search takes one of a query, a batch of queries and a PSSM");
    if ((hits && rq.pssm) || (rq.evalue && !hits) || (rq.ranked && !rq.evalue))
        throw std::invalid_argument("significances belong to a hit table, ranking by them to significances, "
                                    "and a hit table to a query or a batch");
    if (batch && (k < 1 || k > 4096)) throw std::invalid_argument("a batch of queries needs 1 <= k <= 4096");
    if (hits && (k < 1 || k > 4096)) throw std::invalid_argument("the hit table needs 1 <= k <= 4096");
    std::lock_guard<std::mutex> lock(g_mu);  // the reference is not re-entrant either
    g_timing = sw_solver_timing{};
    // Subjects and query as written, or with the '/' padding of the parser
    // and of SWSolver.cu:267-269?  The padding scores 0 under the reference's
    // table alone, so a set scoring drops it; a hit table's coordinates are
    // those of the sequences as written; batches and PSSMs never had it.
    const bool as_written = hits || batch || rq.pssm || iter || g_sc.custom;
    Subjects s = fdb ? Subjects(*fdb, as_written && cp == CharPath::NO) : Subjects(file);
    const double t_solve = now_s();  // a loaded file's solve_s: the search once the subjects are in hand
    const int64_t n = s.n();
    const bool no_id = std::any_of(s.ids.begin(), s.ids.end(), [](int32_t id) { return id < 0; });
    if (fdb && no_id && (hits || batch || iter))
        throw std::invalid_argument(batch  ? "a batch of queries needs record ids (a FASTA header per subject)"
                                    : iter ? "an iterated search needs record ids (a FASTA header per subject)"
                                           : "the hit table needs record ids (a FASTA header per subject)");
    // every score to the host: the plain scan, and a top-K ranked there
    const bool host_rank = rq.mode == sw_search_request::TOPK && !iter && (k > 4096 || (fdb && (no_id || n == 0)));
    const bool all_scores = rq.mode == sw_search_request::SCORES || host_rank;

    std::vector<uint8_t> qc;
    std::vector<int64_t> qoffs;
    if (batch) concat_queries(*rq.queries, &qc, &qoffs);
    else if (rq.query) {
        std::string q = *rq.query;
        while (!as_written && cp != CharPath::TABLE && q.size() % TILE_SIZE != 0) q += "/";
        qc = encode(q);
    }
    const int32_t ql = static_cast<int32_t>(qc.size()), nq = batch ? static_cast<int32_t>(rq.queries->size()) : 1;
    int8_t char_mat[625];
    if (cp == CharPath::TABLE) check(sw_builtin_matrix(SW_MATRIX_BLOSUM50_CHAR, char_mat), "sw_builtin_matrix");
    const sw_scoring sc = cp == CharPath::TABLE ? sw_scoring{char_mat, 2, 2}
                                                : sw_scoring{g_sc.has_matrix ? g_sc.mat : nullptr, g_sc.go, g_sc.ge};

    sw_search_result r;
    r.num_subjects = s.num_subjects;
    r.padded_residues = s.padded_sum;
    r.scores.resize(hits ? 0 : static_cast<size_t>(nq));
    // only a FASTA's plain scan and top-K are sharded over several GPUs
    const bool sharded = fdb && rq.query && !hits && !iter && gpus() > 1;
    g_timing.gpus = sharded ? gpus() : 1;
    if (n == 0 && all_scores && !rq.pssm) return r;

    sw_handle* h = nullptr;
    sw_group* g = nullptr;
    {
        Stage init(g_timing.init_s);  // device start-up (HIP runtime, handle or group) is timed on its own
        if (sharded) g = group();
        else h = handle();
    }
    sw_pssm_ptr pssm;
    {
        Stage upload(g_timing.upload_s);
        const int32_t* ids = all_scores ? nullptr : s.ids.data();  // the top-K and the hit table report record ids
        if (fdb && sharded) {
            sw_gdb* gdb = nullptr;
            check(sw_group_db_create(g, s.residues.data(), s.offsets.data(), n, ids, &gdb), "sw_group_db_create");
            s.gdb.reset(gdb);
        } else if (fdb) {
            sw_db* db = nullptr;
            check(sw_db_create(h, s.residues.data(), s.offsets.data(), n, ids, &db), "sw_db_create");
            s.db.reset(db);
        }
        if (rq.pssm) {
            sw_pssm* p = nullptr;
            check(sw_pssm_create(h, rq.pssm->data(), static_cast<int32_t>(rq.pssm->size() / 25), &p), "sw_pssm_create");
            pssm.reset(p);
        }
    }

    const sw_db* db = s.db.get();
    const size_t table = hits ? static_cast<size_t>(nq) * static_cast<size_t>(k) : 0;
    std::vector<int32_t> scores(static_cast<size_t>(all_scores ? (s.from_file ? s.max_id + 1 : n) : 0), 0);
    std::vector<int64_t> keys(all_scores || hits || iter ? 0 : static_cast<size_t>(nq) * static_cast<size_t>(k));
    std::vector<sw_hit> rows(table);
    std::vector<sw_sig> sigs(rq.evalue ? table : 0);
    std::vector<int32_t> nhits(hits ? static_cast<size_t>(nq) : 0, 0);  // a ranked query's row count is its own
    r.calibs.resize(rq.evalue ? static_cast<size_t>(nq) : 0);
    r.n_pass.resize(rq.ranked ? static_cast<size_t>(nq) : 0);
    int rc = SW_OK;
    {
        Stage scan(g_timing.scan_s);
        if (all_scores) {
            if (n == 0) rc = SW_OK;
            else if (rq.pssm) rc = sw_scan_pssm(h, db, pssm.get(), g_sc.go, g_sc.ge, scores.data());
            else if (sharded) rc = sw_group_scan(g, s.gdb.get(), qc.data(), ql, &sc, scores.data());
            else rc = sw_scan(h, db, qc.data(), ql, &sc, scores.data());
        } else if (iter) {
            // the iterated search (sw_amd.h sw_search_iter): the report in E-value order, the
            // rounds' trace and the last round's profile with the query as its consensus
            std::vector<int32_t> ids(static_cast<size_t>(k)), sco(static_cast<size_t>(k));
            r.iter_sigs.resize(static_cast<size_t>(k));
            r.rounds.resize(static_cast<size_t>(rq.iterations));
            int32_t m = 0, run = 0, conv = 0;
            sw_pssm* last = nullptr;
            rc = sw_search_iter(h, db, qc.data(), ql, &sc, rq.iterations, rq.inclusion_evalue, 4096, 10.0, k, rq.max_evalue,
                                ids.data(), sco.data(), r.iter_sigs.data(), &m, &r.iter_n_pass, &r.iter_calib,
                                r.rounds.data(), &run, &conv, &last);
            pssm.reset(last);
            if (rc == SW_OK) {
                r.rounds.resize(static_cast<size_t>(run));
                r.iter_sigs.resize(static_cast<size_t>(m));
                r.converged = conv != 0;
                for (int32_t i = 0; i < m; ++i) r.scores[0].push_back(std::make_pair(ids[i], sco[i]));
                r.final_pssm.resize(static_cast<size_t>(ql) * 25);
                rc = sw_pssm_rows(last, r.final_pssm.data());
                r.final_consensus = *rq.query;
            }
        } else if (!hits) {
            if (batch) rc = sw_scan_batch_topk(h, db, qc.data(), qoffs.data(), nq, &sc, k, keys.data());
            else if (rq.pssm) rc = sw_scan_pssm_topk(h, db, pssm.get(), g_sc.go, g_sc.ge, k, keys.data());
            else if (sharded) rc = sw_group_topk(g, s.gdb.get(), qc.data(), ql, &sc, k, keys.data());
            else rc = sw_scan_topk(h, db, qc.data(), ql, &sc, k, keys.data());
        } else if (batch) {
            if (rq.ranked)
                rc = sw_scan_batch_hits_ranked(h, db, qc.data(), qoffs.data(), nq, &sc, k, rq.max_evalue, 0, rows.data(),
                                               sigs.data(), nhits.data(), r.n_pass.data(), r.calibs.data());
            else if (rq.evalue)
                rc = sw_scan_batch_hits_sig(h, db, qc.data(), qoffs.data(), nq, &sc, k, rows.data(), sigs.data(),
                                            nhits.data(), r.calibs.data());
            else rc = sw_scan_batch_hits(h, db, qc.data(), qoffs.data(), nq, &sc, k, rows.data(), nhits.data());
            if (!rq.ranked) std::fill(nhits.begin(), nhits.end(), nhits.empty() ? 0 : nhits[0]);  // one count for all
        } else if (rq.ranked) {
            rc = sw_scan_hits_ranked(h, db, qc.data(), ql, &sc, k, rq.max_evalue, rows.data(), sigs.data(), nhits.data(),
                                     r.n_pass.data(), r.calibs.data());
        } else if (rq.evalue) {
            rc = sw_scan_hits_sig(h, db, qc.data(), ql, &sc, k, rows.data(), sigs.data(), nhits.data(), r.calibs.data());
        } else {
            rc = sw_scan_hits(h, db, qc.data(), ql, &sc, k, rows.data(), nhits.data());
        }
    }
    check(rc, entry_name(rq, s.from_file, sharded, all_scores).c_str());

    if (all_scores) {
        r.scores[0].reserve(static_cast<size_t>(n));
        for (int64_t i : s.order)
            r.scores[0].push_back(std::make_pair(static_cast<int>(s.ids[static_cast<size_t>(i)]),
                                                 static_cast<int>(scores[static_cast<size_t>(s.score_slot(i))])));
        if (host_rank) rank_on_host(&r.scores[0], k);
    }
    for (size_t q = 0; q < static_cast<size_t>(nq) && !keys.empty(); ++q)
        for (int i = 0; i < k && keys[q * static_cast<size_t>(k) + i] != INT64_MIN; ++i)
            r.scores[q].push_back(decode_key(keys[q * static_cast<size_t>(k) + i]));
    for (size_t q = 0; q < nhits.size(); ++q) {
        r.rows.push_back(rows_of(rows, q, k, nhits[q]));
        if (rq.evalue) r.sigs.push_back(rows_of(sigs, q, k, nhits[q]));
    }
    r.solve_s = now_s() - t_solve;
    return r;
}

sw_search_request request(const std::string* query, const std::vector<std::string>* queries,
                          const std::vector<int8_t>* pssm, sw_search_request::Mode mode, int k) {
    sw_search_request rq = {};
    rq.query = query;
    rq.queries = queries;
    rq.pssm = pssm;
    rq.mode = mode;
    rq.k = k;
    return rq;
}

// One matrix entry of a text matrix file.
bool parse_int(const std::string& tok, int* v) {
    char* end = nullptr;
    const long x = std::strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end != '\0' || x < -100 || x > 100) return false;
    *v = static_cast<int>(x);
    return true;
}

}  // namespace

bool sw_solver_read_matrix(const std::string& spec, int8_t out[625], std::string* err) {
    std::string low(spec);
    for (char& c : low) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
    if (low == "blosum50") return sw_builtin_matrix(SW_MATRIX_BLOSUM50_REF, out) == SW_OK;
    if (low == "blosum62") return sw_builtin_matrix(SW_MATRIX_BLOSUM62, out) == SW_OK;
    auto bad = [&](const std::string& why) {
        if (err) *err = spec + ": " + why;
        return false;
    };
    std::ifstream in(spec.c_str());
    if (!in) return bad("cannot open matrix file (or use blosum50 / blosum62)");
    static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";  // code order (SWSolver.cu:17-41)
    auto code_of = [&](const std::string& t) -> int {
        if (t.size() != 1) return -1;
        const char* p = std::strchr(kLetters, std::toupper(static_cast<unsigned char>(t[0])));
        return p && *p ? static_cast<int>(p - kLetters) : -1;
    };
    std::vector<std::vector<std::string>> rows;
    std::string line;
    while (std::getline(in, line)) {
        const size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        std::istringstream ls(line);
        std::vector<std::string> tok;
        for (std::string t; ls >> t;) tok.push_back(t);
        if (!tok.empty()) rows.push_back(tok);
    }
    if (rows.empty()) return bad("empty matrix file");
    int v = 0;
    if (parse_int(rows[0][0], &v)) {  // 25 rows of 25 numbers in code order
        if (rows.size() != 25) return bad("expected 25 rows of 25 numbers (code order ARNDCQEGHILKMFPSTWYVBJZX*)");
        for (int a = 0; a < 25; ++a) {
            if (rows[a].size() != 25) return bad("expected 25 numbers in row " + std::to_string(a + 1));
            for (int b = 0; b < 25; ++b) {
                if (!parse_int(rows[a][b], &v)) return bad("bad entry '" + rows[a][b] + "' (integers in -100..100)");
                out[a * 25 + b] = static_cast<int8_t>(v);
            }
        }
        return true;
    }
    // NCBI layout: a header row of residue letters, then one row per letter
    std::vector<int> col;
    for (const std::string& t : rows[0]) {
        const int c = code_of(t);
        if (c < 0) return bad("unknown residue letter '" + t + "' in the header row");
        col.push_back(c);
    }
    int16_t m[25][25];
    bool have[25] = {};
    for (size_t r = 1; r < rows.size(); ++r) {
        const int a = code_of(rows[r][0]);
        if (a < 0) return bad("unknown residue letter '" + rows[r][0] + "'");
        if (rows[r].size() != col.size() + 1) return bad("row '" + rows[r][0] + "' does not match the header");
        if (have[a]) return bad("row '" + rows[r][0] + "' given twice");
        for (size_t j = 0; j < col.size(); ++j) {
            if (!parse_int(rows[r][j + 1], &v)) return bad("bad entry '" + rows[r][j + 1] + "' (integers in -100..100)");
            m[a][col[j]] = static_cast<int16_t>(v);
        }
        have[a] = true;
    }
    bool in_cols[25] = {};
    for (int c : col) in_cols[c] = true;
    for (int a = 0; a < 25; ++a)
        if (have[a] != in_cols[a]) return bad(std::string("letter '") + kLetters[a] + "' is a row or a column, not both");
    // letters the file leaves out (e.g. J in NCBI BLOSUM62) score as X
    constexpr int X = 23;
    for (int a = 0; a < 25; ++a)
        if (!have[a] && !have[X]) return bad(std::string("no row for '") + kLetters[a] + "' and no X row to stand in");
    for (int a = 0; a < 25; ++a)
        for (int b = 0; b < 25; ++b) out[a * 25 + b] = static_cast<int8_t>(m[have[a] ? a : X][have[b] ? b : X]);
    return true;
}

// The PSSM text format (sw_solver_ext.h; pssm.py restates this parser).
bool sw_solver_read_pssm(const std::string& path, std::vector<int8_t>* rows, std::string* consensus,
                         std::string* err) {
    auto bad = [&](const std::string& why) {
        if (err) *err = path + ": " + why;
        return false;
    };
    std::ifstream in(path.c_str());
    if (!in) return bad("cannot open PSSM file");
    static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";  // code order (SWSolver.cu:17-41)
    auto is_letter = [](const std::string& t) {
        return t.size() == 1 && (std::isalpha(static_cast<unsigned char>(t[0])) || t[0] == '*');
    };
    auto code_of = [&](const std::string& t) -> int {
        const char* p = std::strchr(kLetters, std::toupper(static_cast<unsigned char>(t[0])));
        return p && *p ? static_cast<int>(p - kLetters) : -1;
    };
    auto is_int = [](const std::string& t) {
        size_t k = (t[0] == '+' || t[0] == '-') ? 1 : 0;
        if (k == t.size()) return false;
        for (; k < t.size(); ++k)
            if (!std::isdigit(static_cast<unsigned char>(t[k]))) return false;
        return true;
    };
    std::vector<int> col;  // the code of each named column
    bool named[25] = {};
    bool header = false;
    if (rows) rows->clear();
    if (consensus) consensus->clear();
    size_t nrows = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::vector<std::string> tok;
        for (std::string t; ls >> t;) tok.push_back(t);
        if (tok.empty() || tok[0][0] == '#') continue;
        if (!header) {
            bool all = true;
            for (const std::string& t : tok) all = all && is_letter(t);
            if (!all) continue;  // lines before the header
            for (const std::string& t : tok) {
                const int c = code_of(t);
                if (c < 0) return bad("unknown residue letter '" + t + "' in the header");
                if (named[c]) break;  // NCBI repeats the letters for its percentage columns
                named[c] = true;
                col.push_back(c);
            }
            header = true;
            continue;
        }
        // a row: [position] [consensus letter] scores...; without a letter a
        // leading position is recognised by the row holding more tokens than columns
        size_t at = 0;
        bool pos = false;
        int cons = -1;
        if (tok.size() >= 2 && is_int(tok[0]) && is_letter(tok[1])) {
            pos = true;
            at = 1;
        }
        if (at < tok.size() && is_letter(tok[at])) {
            cons = code_of(tok[at]);
            if (cons < 0) return bad("unknown residue letter '" + tok[at] + "'");
            ++at;
        } else if (is_int(tok[0]) && tok.size() > col.size()) {
            pos = true;
            at = 1;
        }
        if (at >= tok.size()) {
            if (pos) return bad("short row '" + line + "'");
            break;
        }
        if (!is_int(tok[at])) break;  // not a row: the table has ended
        if (tok.size() - at < col.size())
            return bad("short row " + std::to_string(nrows + 1) + ": " + std::to_string(tok.size() - at) + " of " +
                       std::to_string(col.size()) + " entries");
        int v[25];
        int lo = 101;
        for (size_t j = 0; j < col.size(); ++j) {
            const std::string& t = tok[at + j];
            if (!is_int(t)) return bad("bad entry '" + t + "' in row " + std::to_string(nrows + 1));
            const long x = t.size() > 5 ? 1000 : std::strtol(t.c_str(), nullptr, 10);
            if (x < -100 || x > 100) return bad("entry '" + t + "' outside -100..100 in row " + std::to_string(nrows + 1));
            v[col[j]] = static_cast<int>(x);
            lo = std::min(lo, v[col[j]]);
        }
        // unnamed columns: B, Z, J from their pairs, the rest from X or the row's minimum
        bool have[25];
        std::memcpy(have, named, sizeof have);
        static const int kPair[3][3] = {{20, 2, 3}, {22, 5, 6}, {21, 9, 10}};  // B: N D, Z: Q E, J: I L
        for (const auto& p : kPair)
            if (!named[p[0]] && named[p[1]] && named[p[2]]) {
                const int s = v[p[1]] + v[p[2]];
                v[p[0]] = s >= 0 ? s / 2 : -((-s + 1) / 2);  // floor
                have[p[0]] = true;
            }
        for (int c = 0; c < 25; ++c)
            if (!have[c]) v[c] = named[23] ? v[23] : lo;
        if (cons < 0) {  // no consensus given: the best-scoring named column (first in code order)
            for (int c = 0; c < 25; ++c)
                if (named[c] && (cons < 0 || v[c] > v[cons])) cons = c;
        }
        if (rows)
            for (int c = 0; c < 25; ++c) rows->push_back(static_cast<int8_t>(v[c]));
        if (consensus) consensus->push_back(kLetters[cons]);
        ++nrows;
    }
    if (!header) return bad("no header line of residue letters");
    if (nrows == 0) return bad("no rows after the header");
    return true;
}

bool sw_solver_write_pssm(const std::string& path, const std::vector<int8_t>& rows, const std::string& consensus,
                          std::string* err) {
    auto bad = [&](const std::string& why) {
        if (err) *err = path + ": " + why;
        return false;
    };
    static const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";
    const size_t n = rows.size() / 25;
    if (rows.size() % 25 != 0 || n == 0) return bad("a PSSM is [positions][25], positions >= 1");
    if (!consensus.empty() && consensus.size() != n) return bad("the consensus has one letter per position");
    for (int8_t v : rows)
        if (v < -100 || v > 100) return bad("entries must be in -100..100");
    std::ofstream out(path.c_str());
    if (!out) return bad("cannot open PSSM file for writing");
    out << "# position-specific scoring matrix: position, consensus, one score per residue code\n ";
    for (int c = 0; c < 25; ++c) out << "   " << kLetters[c];
    out << "\n";
    for (size_t i = 0; i < n; ++i) {
        // the consensus as the reader maps it: a letter of the alphabet, else '*'; none given: the best column
        int cons = 0;
        if (!consensus.empty()) {
            const char* p = std::strchr(kLetters, std::toupper(static_cast<unsigned char>(consensus[i])));
            cons = p && *p ? static_cast<int>(p - kLetters) : 24;
        } else {
            for (int c = 1; c < 25; ++c)
                if (rows[i * 25 + c] > rows[i * 25 + cons]) cons = c;
        }
        out << (i + 1) << " " << kLetters[cons];
        for (int c = 0; c < 25; ++c) out << " " << static_cast<int>(rows[i * 25 + c]);
        out << "\n";
    }
    out.flush();
    if (!out) return bad("write failed");
    return true;
}

bool sw_solver_read_queries(const std::string& path, std::vector<std::string>* names, std::vector<std::string>* seqs,
                            std::string* err) {
    auto bad = [&](const std::string& why) {
        if (err) *err = path + ": " + why;
        return false;
    };
    std::ifstream in(path.c_str());
    if (!in) return bad("cannot open query file");
    std::vector<std::string> nm, sq;
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') {
            const size_t a = line.find_first_not_of(" \t", 1);
            const size_t b = a == std::string::npos ? a : line.find_first_of(" \t\r", a);
            nm.push_back(a == std::string::npos ? std::string() : line.substr(a, b == std::string::npos ? b : b - a));
            sq.emplace_back();
            continue;
        }
        for (char c : line) {
            if (std::isspace(static_cast<unsigned char>(c))) continue;
            if (sq.empty()) return bad("residues before the first '>' line");
            sq.back() += c;
        }
    }
    if (sq.empty()) return bad("no '>' line: not a FASTA file");
    if (names) names->swap(nm);
    if (seqs) seqs->swap(sq);
    return true;
}

void sw_solver_set_scoring(const int8_t* matrix625, int gap_open, int gap_extend) {
    if (gap_open < 1 || gap_open > 1000 || gap_extend < 1 || gap_extend > 1000)
        throw std::invalid_argument("gap penalties must be in 1..1000");
    if (matrix625)
        for (int k = 0; k < 625; ++k)
            if (matrix625[k] < -100 || matrix625[k] > 100)
                throw std::invalid_argument("matrix entries must be in -100..100");
    std::lock_guard<std::mutex> lock(g_mu);
    g_sc = SolverScoring{};
    g_sc.custom = true;
    g_sc.has_matrix = matrix625 != nullptr;
    if (matrix625) std::memcpy(g_sc.mat, matrix625, 625);
    g_sc.go = gap_open;
    g_sc.ge = gap_extend;
}

void sw_solver_reset_scoring() {
    std::lock_guard<std::mutex> lock(g_mu);
    g_sc = SolverScoring{};
}

sw_search_result sw_solver_search(const std::string& db_path, const sw_search_request& rq) {
    if (db_path.size() > 5 && db_path.compare(db_path.size() - 5, 5, ".swdb") == 0) return search(nullptr, db_path, rq);
    const double t0 = now_s();
    FASTADatabase fdb(db_path);
    const double parse_s = now_s() - t0;
    const double t1 = now_s();
    sw_search_result r = search(&fdb, std::string(), rq);
    r.parse_s = parse_s;
    r.solve_s = now_s() - t1;  // a FASTA's: flatten, upload, scan, and the database freed again
    return r;
}

void smith_waterman_cuda(FASTAQuery& query, FASTADatabase& db, std::vector<seqid_score>& result) {
    const std::string q = query.get_buffer();
    const sw_search_result r = search(&db, std::string(), request(&q, nullptr, nullptr, sw_search_request::SCORES, 0));
    result.insert(result.end(), r.scores[0].begin(), r.scores[0].end());
}

// Scores equal smith_waterman_cuda's (golden-pinned), returned in file order;
// SW_CHAR_COMPAT=1 scores with the _char path's own table instead
// (SW_MATRIX_BLOSUM50_CHAR).
std::vector<seqid_score> smith_waterman_cuda_char(FASTAQuery& query, FASTADatabase& db) {
    const std::string q = query.get_buffer();
    const char* cc = std::getenv("SW_CHAR_COMPAT");
    std::vector<seqid_score> out = search(&db, std::string(), request(&q, nullptr, nullptr, sw_search_request::SCORES, 0),
                                          cc && cc[0] == '1' ? CharPath::TABLE : CharPath::ORDER).scores[0];
    std::stable_sort(out.begin(), out.end(),
                     [](const seqid_score& a, const seqid_score& b) { return a.first < b.first; });
    return out;
}

std::vector<seqid_score> smith_waterman_cuda_topk(FASTAQuery& query, FASTADatabase& db, int k) {
    if (k < 1) throw std::invalid_argument("top-k needs k >= 1");
    const std::string q = query.get_buffer();
    return search(&db, std::string(), request(&q, nullptr, nullptr, sw_search_request::TOPK, k)).scores[0];
}

std::vector<seqid_score> smith_waterman_cuda_pssm(const std::vector<int8_t>& rows, FASTADatabase& db, int k) {
    if (k < 0) throw std::invalid_argument("top-k needs k >= 0");
    if (rows.size() % 25 != 0) throw std::invalid_argument("a PSSM holds 25 entries per row");
    const sw_search_request::Mode mode = k ? sw_search_request::TOPK : sw_search_request::SCORES;
    return search(&db, std::string(), request(nullptr, nullptr, &rows, mode, k)).scores[0];
}

namespace {
// The hit-table entry points: one query (seqs null) or a batch; `evalue` asks
// for significances and calibrations, `ranked` for the E-value order as well.
sw_search_result hits_search(const std::string* query, const std::vector<std::string>* seqs, FASTADatabase& db, int k,
                             bool evalue, bool ranked, double max_evalue) {
    sw_search_request rq = request(query, seqs, nullptr, sw_search_request::HITS, k);
    rq.evalue = evalue;
    rq.ranked = ranked;
    rq.max_evalue = max_evalue;
    return search(&db, std::string(), rq);
}
}  // namespace

namespace {
// The three one-query forms: sig null for the plain table; `ranked` for the E-value order.
std::vector<sw_hit> query_hits(FASTAQuery& query, FASTADatabase& db, int k, bool ranked, double max_evalue,
                               std::vector<sw_sig>* sig, int64_t* n_pass, sw_calib* calib) {
    const std::string q = query.get_buffer();
    sw_search_result r = hits_search(&q, nullptr, db, k, sig != nullptr, ranked, max_evalue);
    if (sig) sig->swap(r.sigs[0]);
    if (sig && calib) *calib = r.calibs[0];
    if (ranked && n_pass) *n_pass = r.n_pass[0];
    return r.rows[0];
}
}  // namespace

std::vector<sw_hit> smith_waterman_cuda_hits(FASTAQuery& query, FASTADatabase& db, int k) {
    return query_hits(query, db, k, false, 0, nullptr, nullptr, nullptr);
}

std::vector<sw_hit> smith_waterman_cuda_hits_sig(FASTAQuery& query, FASTADatabase& db, int k, std::vector<sw_sig>* sig,
                                                 sw_calib* calib) {
    if (!sig) throw std::invalid_argument("smith_waterman_cuda_hits_sig needs a vector for the significances");
    return query_hits(query, db, k, false, 0, sig, nullptr, calib);
}

std::vector<sw_hit> smith_waterman_cuda_hits_ranked(FASTAQuery& query, FASTADatabase& db, int k, double max_evalue,
                                                    std::vector<sw_sig>* sig, int64_t* n_pass, sw_calib* calib) {
    if (!sig) throw std::invalid_argument("smith_waterman_cuda_hits_ranked needs a vector for the significances");
    return query_hits(query, db, k, true, max_evalue, sig, n_pass, calib);
}

std::vector<std::vector<seqid_score>> smith_waterman_cuda_batch_topk(const std::vector<std::string>& seqs,
                                                                     FASTADatabase& db, int k) {
    return search(&db, std::string(), request(nullptr, &seqs, nullptr, sw_search_request::TOPK, k)).scores;
}

std::vector<std::vector<sw_hit>> smith_waterman_cuda_batch_hits(const std::vector<std::string>& seqs,
                                                                FASTADatabase& db, int k) {
    return hits_search(nullptr, &seqs, db, k, false, false, 0).rows;
}

std::vector<std::vector<sw_hit>> smith_waterman_cuda_batch_hits_sig(const std::vector<std::string>& seqs,
                                                                    FASTADatabase& db, int k,
                                                                    std::vector<std::vector<sw_sig>>* sig,
                                                                    std::vector<sw_calib>* calib) {
    if (!sig || !calib) throw std::invalid_argument("smith_waterman_cuda_batch_hits_sig needs its two output vectors");
    sw_search_result r = hits_search(nullptr, &seqs, db, k, true, false, 0);
    sig->swap(r.sigs);
    calib->swap(r.calibs);
    return r.rows;
}

std::vector<std::vector<sw_hit>> smith_waterman_cuda_batch_hits_ranked(const std::vector<std::string>& seqs,
                                                                       FASTADatabase& db, int k, double max_evalue,
                                                                       std::vector<std::vector<sw_sig>>* sig,
                                                                       std::vector<int64_t>* n_pass,
                                                                       std::vector<sw_calib>* calib) {
    if (!sig || !n_pass || !calib)
        throw std::invalid_argument("smith_waterman_cuda_batch_hits_ranked needs its three output vectors");
    sw_search_result r = hits_search(nullptr, &seqs, db, k, true, true, max_evalue);
    sig->swap(r.sigs);
    n_pass->swap(r.n_pass);
    calib->swap(r.calibs);
    return r.rows;
}

void sw_save_fasta_db(FASTADatabase& fdb, const std::string& path) {
    std::lock_guard<std::mutex> lock(g_mu);
    const Subjects s(fdb, true);  // as written; a search of the file restores the padded sizes for METRICS
    sw_db* made = nullptr;
    check(sw_db_create(handle(), s.residues.data(), s.offsets.data(), s.n(), s.n() ? s.ids.data() : nullptr, &made),
          "sw_db_create");
    const sw_db_ptr db(made);
    check(sw_db_save(db.get(), path.c_str()), "sw_db_save");
}

void sw_solver_set_gpus(int n) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (n != g_gpus) g_group.reset();
    g_gpus = n;
}

sw_group* sw_solver_group() {
    std::lock_guard<std::mutex> lock(g_mu);
    return gpus() > 1 ? group() : nullptr;
}

sw_solver_timing sw_solver_last_timing() { return g_timing; }
