/*
 * sw_solver_ext.h — additions of this build to the C++ drop-in (SWSolver.h
 * itself stays identical to the reference's src/SWSolver.h:7,9).  Used by
 * lib/main and lib/sw_tests; the reference has no counterpart.
 */
#ifndef SW_SOLVER_EXT_H
#define SW_SOLVER_EXT_H

#include <stdint.h>

#include <string>
#include <vector>

#include "FASTAParsers.h"
#include "SWSolver.h"
#include "sw_amd.h"

/* Wall time of the last smith_waterman_cuda[_char] call, split as
 * flatten (map walk + encode on the host's cores), upload (pack + H2D into
 * resident shards) and scan (kernels + D2H of the scores). */
struct sw_solver_timing {
    double flatten_s;
    double upload_s;  /* sw_db_create: host packing + H2D of the database */
    double scan_s;
    int gpus;
    double init_s;    /* device start-up (HIP runtime, handle / group): the first call only */
};
sw_solver_timing sw_solver_last_timing();

/* Devices smith_waterman_cuda shards the database over (default: $SW_GPUS,
 * else 1; `main --gpus N`).  1 = the single-handle path. */
void sw_solver_set_gpus(int n);
/* The process-wide group behind the N > 1 path (created on first use), or
 * NULL when the solver runs on one GPU. */
sw_group* sw_solver_group();

/* main --make-db: the flattened database (reference order, record ids as
 * result ids, subjects as written: no '/' padding) written as a sw_db_save
 * file. */
void sw_save_fasta_db(FASTADatabase& fdb, const std::string& path);

/* Scoring of smith_waterman_cuda / smith_waterman_cuda_topk (the reference
 * hard-wires BLOSUM50, SWSolver.cu:54-81, and GAP_PENALTY 2, SWSolver.cu:7,
 * with "define affine penalty ?" left open at :8).  matrix625: 25x25 int8 in
 * code order (sw_amd.h), NULL = the reference's BLOSUM50; a gap of k
 * residues costs gap_open + (k - 1) gap_extend (open == extend: linear).
 * Throws std::invalid_argument outside 1..1000 / -100..100.  Until it is
 * called (or after sw_solver_reset_scoring) the solver scores exactly as the
 * reference, query padding included; a set scoring scans the query and
 * the subjects as written (without the '/' padding of SWSolver.cu:267-269
 * and FASTAParsers.h, which scores 0 only under the reference's table). */
void sw_solver_set_scoring(const int8_t* matrix625, int gap_open, int gap_extend);
void sw_solver_reset_scoring();
/* `spec` = "blosum50" (the reference's table), "blosum62", or a text file:
 * either 25 rows of 25 integers in code order ARNDCQEGHILKMFPSTWYVBJZX*, or
 * the NCBI layout (a header row of residue letters, then one row per letter,
 * '#' comments); letters an NCBI file leaves out (J in NCBI's BLOSUM62) score
 * as its X row / column.  False (and *err) on a bad file. */
bool sw_solver_read_matrix(const std::string& spec, int8_t out[625], std::string* err);

/* The k best subjects of the database for this query, score descending then
 * record id ascending, as (record id, score) pairs — the scan plus a device
 * top-K (sw_scan_topk; with several GPUs sw_group_topk: per-device top-K and
 * one RCCL all-gather), so only k results leave the GPU.  Fewer than k when
 * the database is smaller.  k > 4096 ranks every score on the host. */
std::vector<seqid_score> smith_waterman_cuda_topk(FASTAQuery& query, FASTADatabase& db, int k);

/* The hit table (sw_amd.h sw_scan_hits; `main --hits K`): the k best subjects
 * in smith_waterman_cuda_topk's order, each as a sw_hit row — the record id
 * and score, where the alignment lies in the query and in the subject
 * (1-based, inclusive), the subject's length, the alignment's length,
 * identities, positives, gap runs and gap columns — under the scoring of
 * sw_solver_set_scoring (default: the reference's).  Coordinates are those of
 * the sequences as written: neither the subjects nor the query carry the '/'
 * padding (it scores 0 under the reference's table, so the scores are the
 * ranked scan's).  1 <= k <= 4096; fewer rows when the database is smaller.
 * One GPU.  Throws std::invalid_argument for another k or a subject without
 * a record id. */
std::vector<sw_hit> smith_waterman_cuda_hits(FASTAQuery& query, FASTADatabase& db, int k);
/* The same with each row's E-value, bit score and z-score in (*sig)[i] and
 * the scan's calibration in *calib (may be NULL), from the scan's own scores
 * (sw_amd.h sw_scan_hits_sig; `main --hits K --evalue`). */
std::vector<sw_hit> smith_waterman_cuda_hits_sig(FASTAQuery& query, FASTADatabase& db, int k, std::vector<sw_sig>* sig,
                                                 sw_calib* calib);
/* The same ranked by E-value instead of raw score, with an E-value cutoff
 * (sw_amd.h sw_scan_hits_ranked; `main --hits K --evalue --rank evalue
 * [--max-evalue X]`): the rows of the min(k, *n_pass) most significant
 * subjects with E <= max_evalue (+infinity: no cutoff), in E-value order;
 * *n_pass (may be NULL), the subjects that pass, may exceed k. */
std::vector<sw_hit> smith_waterman_cuda_hits_ranked(FASTAQuery& query, FASTADatabase& db, int k, double max_evalue,
                                                    std::vector<sw_sig>* sig, int64_t* n_pass, sw_calib* calib);

/* Batches of queries (sw_amd.h sw_scan_batch_topk / sw_scan_batch_hits;
 * `main --queries FILE`).  sw_solver_read_queries reads a multi-record FASTA
 * file: each line starting with '>' opens a record, named by the header's
 * first word (empty when there is none); the lines up to the next '>' are its
 * residues, white space and blank lines dropped; a record may hold none.
 * False and *err when the file cannot be opened, holds no '>' line, or has
 * residues before the first one.
 * smith_waterman_cuda_batch_topk / _batch_hits return, per query in the
 * order given, what smith_waterman_cuda_topk / _hits return for it, from one
 * call of the library: the queries as written (no '/' padding, as
 * smith_waterman_cuda_hits), the subjects as written, under the scoring of
 * sw_solver_set_scoring.  1 <= k <= 4096; one GPU; std::invalid_argument for
 * another k or a subject without a record id. */
bool sw_solver_read_queries(const std::string& path, std::vector<std::string>* names, std::vector<std::string>* seqs,
                            std::string* err);
std::vector<std::vector<seqid_score> > smith_waterman_cuda_batch_topk(const std::vector<std::string>& seqs,
                                                                      FASTADatabase& db, int k);
std::vector<std::vector<sw_hit> > smith_waterman_cuda_batch_hits(const std::vector<std::string>& seqs,
                                                                 FASTADatabase& db, int k);
/* The same with every row's significance in (*sig)[query][i] and every
 * query's calibration in (*calib)[query] (sw_amd.h sw_scan_batch_hits_sig). */
std::vector<std::vector<sw_hit> > smith_waterman_cuda_batch_hits_sig(const std::vector<std::string>& seqs,
                                                                     FASTADatabase& db, int k,
                                                                     std::vector<std::vector<sw_sig> >* sig,
                                                                     std::vector<sw_calib>* calib);
/* The batch form of smith_waterman_cuda_hits_ranked (sw_amd.h
 * sw_scan_batch_hits_ranked): (*n_pass)[query] as above; a query's row count
 * is its own. */
std::vector<std::vector<sw_hit> > smith_waterman_cuda_batch_hits_ranked(const std::vector<std::string>& seqs,
                                                                        FASTADatabase& db, int k, double max_evalue,
                                                                        std::vector<std::vector<sw_sig> >* sig,
                                                                        std::vector<int64_t>* n_pass,
                                                                        std::vector<sw_calib>* calib);

/* Profile (PSSM) queries (sw_amd.h sw_pssm_*; `main --pssm FILE`).
 * sw_solver_read_pssm reads a text PSSM into rows ([positions][25] int8 in
 * code order) and its consensus (one letter per position):
 *   - blank lines and lines starting with '#' are ignored, and so is every
 *     line before the header;
 *   - the header is the first line whose tokens are all single residue
 *     letters; its columns are the leading run of distinct letters, stopping
 *     at the first repeat (an NCBI ASCII PSSM repeats its 20 letters for the
 *     percentage columns);
 *   - each following line is one position: an optional integer position, an
 *     optional residue letter (the consensus; without one, the best-scoring
 *     named column), then at least one integer per column; further tokens are
 *     ignored.  Without a letter, a leading position is recognised by the line
 *     holding more tokens than the header has columns;
 *   - the first line that is not such a row ends the table;
 *   - columns the header does not name: B, Z and J take floor((a + b) / 2) of
 *     their pair (N/D, Q/E, I/L) when both are named; every other one takes
 *     the X column when X is named, else the row's minimum.
 * False and *err on a bad file: "no header", "unknown residue letter",
 * "short row", "bad entry", "-100..100", "no rows".
 * smith_waterman_cuda_pssm scans the database with the table in the query's
 * place, under the gaps of sw_solver_set_scoring (default 2/2), subjects as
 * written; k = 0: every subject in the reference's report order, k > 0: the
 * k best (score descending, record id ascending).  One GPU.
 * sw_solver_write_pssm writes such a file: a '#' line, a header naming all 25
 * codes, and per position its number, its consensus letter (consensus[i]; a
 * byte outside the alphabet is written as '*'; an empty consensus: the
 * best-scoring column, first in code order) and 25 scores, so that reading the
 * file back gives the same rows and the same consensus.  False and *err for a
 * table that is not [positions >= 1][25] within -100..100, a consensus of
 * another length, or a file that cannot be written.
 * Out of scope: batches of PSSMs, several GPUs (sw_group_*), sw_score_pair,
 * position-specific gap costs.  Building a PSSM from hits: the iterated
 * search below. */
bool sw_solver_read_pssm(const std::string& path, std::vector<int8_t>* rows, std::string* consensus,
                         std::string* err);
bool sw_solver_write_pssm(const std::string& path, const std::vector<int8_t>& rows, const std::string& consensus,
                          std::string* err);
std::vector<seqid_score> smith_waterman_cuda_pssm(const std::vector<int8_t>& rows, FASTADatabase& db,
                                                  int k /* 0 = all, in the reference's report order */);

/* The one search behind every function above, and `main`'s only one: what is
 * searched for (exactly one of query, queries and pssm is non-null), which
 * result is wanted, and the database by path, a FASTA file or a .swdb file
 * (sw_save_fasta_db).  Per query, in the order given: scores (SCORES: every
 * subject in the reference's report order; TOPK: the k best) or rows (HITS),
 * with sigs and calibs under `evalue`, in E-value order with n_pass under
 * `ranked` (needs evalue; max_evalue as smith_waterman_cuda_hits_ranked's).
 * A .swdb file is scanned on one GPU whatever sw_solver_set_gpus says.
 * The iterated search (sw_amd.h sw_search_iter; `main --iterations N`):
 * iterations > 0 with a query, TOPK and k in 1..4096 (no evalue / ranked, one
 * GPU, record ids): up to `iterations` rounds under inclusion_evalue, every
 * included subject (up to 4096) and a pseudocount weight of 10; scores[0]
 * holds the min(k, iter_n_pass) most significant subjects with E <= max_evalue
 * (> 0; +infinity: no cutoff) of the last round in E-value order, iter_sigs
 * their significances, rounds the trace, final_pssm / final_consensus the last
 * round's profile and the query's letters (sw_solver_write_pssm's arguments).
 * Throws what the functions above throw. */
struct sw_search_request {
    const std::string* query;                /* the residues as written */
    const std::vector<std::string>* queries; /* a batch: HITS or TOPK, k in 1..4096 */
    const std::vector<int8_t>* pssm;         /* [positions][25]: SCORES or TOPK */
    enum Mode { SCORES, TOPK, HITS } mode;
    int k;
    bool evalue, ranked;
    double max_evalue;
    int iterations;           /* 0: a plain search */
    double inclusion_evalue;  /* a round includes the subjects with E <= this */
};
struct sw_search_result {
    std::vector<std::vector<seqid_score> > scores;
    std::vector<std::vector<sw_hit> > rows;
    std::vector<std::vector<sw_sig> > sigs;
    std::vector<sw_calib> calibs;
    std::vector<int64_t> n_pass;
    /* the iterated search */
    std::vector<sw_iter_round> rounds;
    bool converged = false;
    std::vector<sw_sig> iter_sigs;
    int64_t iter_n_pass = 0;
    sw_calib iter_calib = {};
    std::vector<int8_t> final_pssm;
    std::string final_consensus;
    /* main's METRICS: the FASTA parser's counts (subjects padded to TILE_SIZE),
     * the same for a file; the wall time of parsing a FASTA (0 for a file) and
     * of the search after it (a FASTA's: flatten, upload, scan and freeing the
     * database; a file's: the scan once it is loaded) */
    int64_t num_subjects = 0, padded_residues = 0;
    double parse_s = 0, solve_s = 0;
};
sw_search_result sw_solver_search(const std::string& db_path, const sw_search_request& rq);

#endif /* SW_SOLVER_EXT_H */
