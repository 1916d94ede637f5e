/*
 * sw_amd.h — C ABI of the MI355X Smith-Waterman database-scan library
 * (libswamd.so).  Plain pointers and sizes only; no C++ or torch types.
 *
 * This is the boundary the reference's scan path crosses.  The reference has
 * no FFI of its own: its one entry point is the C++ function
 *
 *     void smith_waterman_cuda(FASTAQuery&, FASTADatabase&,
 *                              std::vector<seqid_score>&);     SWSolver.h:9
 *
 * implemented at SWSolver.cu:266-404, plus the (uncompilable) char variant
 * SWSolver_char.h:9 / SWSolver_char.cu:193-280.  Those C++ signatures are
 * kept unchanged in include/SWSolver.h and include/SWSolver_char.h; they are
 * thin shims over the calls below.  Each call names the part of the
 * reference it replaces.
 *
 * Conventions
 *   - Residues are ENCODED bytes: codes 0..24 for A R N D C Q E G H I L K M F
 *     P S T W Y V B J Z X * (SWSolver.cu:17-41); every other input byte is
 *     '*' = 24 (convertStringToFloat, SWSolver.cu:91-120).  sw_encode()
 *     performs that mapping.
 *   - Scores are int32 (the reference's int16 storage overflows for the
 *     self-hits of the longest shipped queries).
 *   - Every call returns SW_OK (0) or a negative SW_E* code; a HIP failure
 *     is returned as SW_E_HIP and its text is kept for sw_last_error().
 *     Nothing fails silently (the reference checks no CUDA error,
 *     SWSolver.cu:276).
 *   - A handle is bound to one device and owns one HIP stream; calls on one
 *     handle are not re-entrant (neither is the reference: it keeps its
 *     query in __constant__ memory, SWSolver.cu:85-89).
 */
#ifndef SW_AMD_H
#define SW_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libswamd.so is built with -fvisibility=hidden; only these are exported. */
#if defined(SW_AMD_BUILD)
#define SW_API __attribute__((visibility("default")))
#else
#define SW_API
#endif

#define SW_OK 0
#define SW_E_INVALID -1   /* bad argument */
#define SW_E_HIP -2       /* HIP runtime error (see sw_last_error) */
#define SW_E_NOMEM -3     /* host allocation failed */
#define SW_E_NODEVICE -4  /* no HIP device / kernel image for this GPU */
#define SW_E_UNSUPPORTED -5 /* valid request this build does not implement */
#define SW_E_IO -6          /* file could not be read / written / validated */
#define SW_E_DEVICE -7      /* a kernel reported an internal fault: the scores of the
                               handle's scans since the last successful call are not
                               trusted (see sw_last_error).  The device writes a
                               host-mapped word; the asynchronous entry points
                               (sw_scan_device, sw_scan_rank_device, the batch and
                               group forms) return before their kernels end, so a
                               fault is reported by the first call on the handle
                               after the faulting kernel has completed (the
                               synchronous sw_scan / sw_scan_topk / sw_scan_batch
                               report their own) */

#define SW_ALPHABET 25    /* residue codes 0..24 */
#define SW_CODE_STAR 24

/* Built-in substitution matrices (25x25 int8, code order). */
#define SW_MATRIX_BLOSUM50_REF 0  /* SWSolver.cu:54-81 exactly ('*' = 0) */
#define SW_MATRIX_BLOSUM62 1      /* NCBI BLOSUM62 (option, not in the reference) */
#define SW_MATRIX_IDENTITY3 2     /* +3/-3, the cpu.cpp:6-8 scheme */
#define SW_MATRIX_BLOSUM50_CHAR 3 /* the _char path's table (SWSolver_char.cu:22-49) as
                                     its lookup (:106-179) reads it: BLOSUM50_REF with
                                     '*' = -5 and '*'/'*' = 1 (its L->W typo at :35 is
                                     never read: the lookup orders the pair by range) */

typedef struct sw_scoring {
    const int8_t* matrix;  /* 625 int8 (row = query code, col = subject code);
                              NULL = SW_MATRIX_BLOSUM50_REF */
    int32_t gap_open;      /* cost of the first residue of a gap (> 0) */
    int32_t gap_extend;    /* cost of each further residue (> 0); equal to
                              gap_open = the reference's linear gap
                              (GAP_PENALTY 2, SWSolver.cu:7) */
} sw_scoring;

typedef struct sw_db_stats {
    int64_t n_subjects;      /* records in the database */
    int64_t residues;        /* sum of unpadded subject lengths */
    int64_t packed_cells;    /* residue columns actually scanned (64 lanes x
                                padded block widths) */
    int64_t n_blocks;        /* 64-subject blocks scanned by the inter-sequence kernel */
    int64_t n_long;          /* subjects routed to the intra-sequence kernel */
    int64_t device_bytes;    /* HBM held by the packed database */
    int32_t max_length;      /* longest subject */
    int32_t long_threshold;  /* subjects longer than this use the intra kernel */
    int32_t coop_blocks;     /* widest blocks the cooperative kernel took in the
                                most recent scan of this database (the split
                                depends on the scoring) */
    int64_t coop_residues;   /* unpadded residues in those blocks */
    int32_t max_id;          /* largest result id (-1 if empty): score arrays hold max_id+1 */
    int32_t pair_blocks;     /* widest blocks run by wave pairs (sw_inter_x2p) in
                                the most recent scan; in the default merged
                                launch they belong to the main inter kernel */
    int32_t pair_merged;     /* 1: pairs and single-wave blocks were one launch */
    int64_t pair_residues;   /* unpadded residues in the pair blocks */
} sw_db_stats;

typedef struct sw_timing {
    float inter_ms;     /* inter-sequence kernel(s), HIP events on the handle's stream */
    float intra_ms;     /* intra-sequence kernel(s) */
    float total_ms;     /* first launch to last completion of the last scan */
    int32_t rescued;    /* subjects re-scored at int32 after an int16 saturation */
    int32_t launches;   /* kernel launches in the last scan */
    float coop_ms;      /* cooperative wide-block kernel alone (events on its stream) */
    float wave_ms;      /* per-wave inter kernel alone (events on the handle's stream) */
} sw_timing;
/* A scan run as ONE merged longest-first launch (sw_last_kernel ends in
 * "+lpt": inter blocks and the long subjects' fp16 pass in one grid) reports
 * that launch as inter_ms and wave_ms and 0 as intra_ms.
 * In a batch (sw_scan_batch*), a query's rescue tail (re-scoring of flagged
 * subjects) may run on a tail stream beside the next query's scan: its time
 * is then outside that query's spans and inside a later query's total_ms;
 * the batch's sum covers all of it. */

typedef struct sw_handle sw_handle;
typedef struct sw_db sw_db;

/* ---- housekeeping ---------------------------------------------------- */
SW_API int32_t sw_version(void);                         /* 10000*major + 100*minor + patch */
/* The id of the sources this library was built from (16 hex digits of a
 * SHA-256 over csrc/ and include/, csrc/build_id.py); the Python binding
 * refuses a library whose id differs from the tree's (a stale build).     */
SW_API const char* sw_build_id(void);
SW_API const char* sw_last_error(void);                  /* thread-local text of the last failure */
SW_API int sw_encode(const char* ascii, int64_t n, uint8_t* codes);    /* SWSolver.cu:91-120 */
SW_API int sw_builtin_matrix(int32_t id, int8_t* out625);               /* SWSolver.cu:54-81 */

/* ---- device context ---------------------------------------------------
 * Replaces the reference's implicit CUDA context + default stream
 * (SWSolver.cu:282-288 allocations, :349/:381 synchronisations).        */
SW_API int sw_create(int32_t device, sw_handle** out);
SW_API int sw_destroy(sw_handle* h);
/* The handle's HIP stream (hipStream_t), e.g. to record events on it. */
SW_API void* sw_stream(sw_handle* h);
/* Use an external stream (e.g. torch's current stream); NULL = own stream. */
SW_API int sw_set_stream(sw_handle* h, void* hip_stream);

/* ---- kernel-form overrides ------------------------------------------------
 * The reference fixes every algorithm parameter at compile time (#defines,
 * SWSolver.cu:7,43-50).  This library chooses its kernel forms per scan from
 * the query, the database and the scoring; sw_opts overrides those choices
 * for tests and A/B measurements.  Scores never depend on it: every form is
 * bit-exact.  Every field is -1 (the library's own choice) after
 * sw_opts_init; a handle starts with those values.  The library reads no
 * environment variable on its scan path: sw_opts_from_env is the one place
 * the SW_* variables are read (test and measurement scripts call it).    */
typedef struct sw_opts {
    int32_t size;             /* sizeof(sw_opts), set by sw_opts_init (ABI check) */
    int32_t lpt;              /* 1: one merged longest-first launch (sw_scan_lpt)
                                 whenever the scan's shape allows it; 0: never  SW_LPT */
    int32_t lpt_pipe;         /* long-subject pairs the merged launch runs in the
                                 pipelined form (query chunk per wave)          SW_LPT_PIPE */
    int32_t quad_width;       /* inter blocks at least this wide run by wave quads
                                 in the merged launch (0: none)                SW_QUAD_WIDTH */
    int32_t pair_width;       /* ... by wave pairs (0: none)                   SW_PAIR_WIDTH */
    int32_t pair_group;       /* waves per group (2 or 4) of the separate pair
                                 launch                                        SW_PAIR_GROUP */
    int32_t coop_width;       /* blocks at least this wide go to the cooperative
                                 int32 kernel (int32 scans)                    SW_COOP_WIDTH */
    int32_t coop_skew;        /* 0: the cooperative kernel without its skew    SW_COOP_SKEW */
    int32_t intra_x2;         /* 0: long subjects in int32 only                SW_INTRA_X2 */
    int32_t intra_x2_rows;    /* rows per lane of the packed intra kernel
                                 (4, 6, 8, 10, 12, 16, 20)                     SW_INTRA_X2_RI */
    int32_t intra_i16_first;  /* 0 / 1: never / always run the long subjects'
                                 int16 form first (default: adaptive)          SW_INTRA_I16_FIRST */
    int32_t inter_i16_span;   /* the widest n blocks in int16 first (0: none;
                                 default: adaptive)                            SW_INTER_I16_SPAN */
    int32_t int16_guard;      /* 0: int32 beyond the static int16 bound        SW_INT16_GUARD */
    int32_t rescue_stats;     /* 1: print what the guard bands flagged per scan
                                 (synchronises)                                SW_RESCUE_STATS */
    int32_t tail_pairs;       /* the narrowest n blocks of the merged launch run
                                 by wave pairs (0: none)                       SW_TAIL_PAIRS */
    int32_t lpt_persist;      /* 0: the merged launch with one workgroup per work
                                 item, never one per resident slot taking items
                                 from a counter (default: that form for tables
                                 of 3+ rounds); n >= 2: that form with n
                                 workgroups (tests)                           SW_LPT_PERSIST */
    int32_t lpt_rows;         /* query rows per pass of the merged launch under
                                 linear gaps: 64 or 96 (default 96)           SW_LPT_ROWS */
    int32_t tri_width;        /* under affine gaps, the merged launch's widest group
                                 blocks at least this wide run by 3-wave groups
                                 (two rounds of a 6-pass query, no idle wave),
                                 whose workgroup's fourth wave runs a single-wave
                                 block, instead of quads (0: none; default
                                 0.48 x the long threshold on databases that run
                                 quads)                                      SW_TRI_WIDTH */
    int32_t lpt_pipe_tail;    /* the last n long-subject pairs of the merged
                                 launch (the shortest) run in the pipelined form
                                 too (0: none; default: 2 % of the pairs for
                                 linear scans of databases that run quads)   SW_LPT_PIPE_TAIL */
    int32_t drain_spin;       /* (tests) polls the merged launch's drain spends
                                 waiting for a claimed rescue-list entry before
                                 it gives up and faults (default 2^22; 0: at
                                 once, i.e. the SW_E_DEVICE path)             SW_DRAIN_SPIN */
    char inter_variant[16];   /* inter kernel shape: "" (auto), "32x8", "64x8"
                                 (int32), "y32x8" (int16 two-strips), "f32x8",
                                 "f32x4" (its fp16 form)                       SW_INTER_VARIANT */
    char trace_file[256];     /* per-workgroup timeline of the merged launch
                                 (builds with -DSW_TRACE_BLOCKS only; "" off)  SW_TRACE_FILE */
} sw_opts;
SW_API int sw_opts_init(sw_opts* o);
/* sw_opts_init, then every field whose SW_* variable (above) is set. */
SW_API int sw_opts_from_env(sw_opts* o);
SW_API int sw_set_opts(sw_handle* h, const sw_opts* o);
SW_API int sw_get_opts(const sw_handle* h, sw_opts* o);

/* ---- database -----------------------------------------------------------
 * Replaces the per-call packing loop SWSolver.cu:301-371 (longest-first
 * 32-lane interleave into managed memory, re-done on every query): the
 * database is sorted, packed and uploaded ONCE and stays resident in HBM.
 *   residues : encoded subject residues, concatenated
 *   offsets  : n+1 offsets into residues (offsets[0] = 0)
 *   ids      : n result ids (NULL = 0..n-1); sw_scan writes scores[id]
 * Lengths.  A subject holds 0 .. 2^30 residues (a longer one is refused with
 * SW_E_INVALID); a query is an int32_t count of rows, which the hit table
 * alone bounds (sw_hit_stats and its kin refuse qlen + subject length >=
 * 2^31); every other entry point is bounded by memory only.  sw_align
 * stores (qlen + slen + 1)(qlen + 1) direction bytes per hit, 4.3 GB for a
 * 65,544-row query however short the subject, one launch group per hit from
 * 2^30 bytes on, and fails with SW_E_HIP when that cannot be allocated.
 * Pinned bit for bit against the CPU
 * oracle (tests/test_gpu_lengths.py): subjects of 32,760, 32,768, 35,213,
 * 65,528, 65,536, 65,544 and 70,001 residues in the lanes (a block 70,016
 * columns wide), as long subjects and under the library's own threshold,
 * through every scan form, both rescue chains, the hit table, sw_align, the
 * calibration table and the file format; queries of 32,760, 32,776, 35,213
 * and 65,544 rows through the scans, batches, sw_score_pair, a PSSM, the hit
 * table (129 chunks) and sw_align (direction arrays past 2^30 and 2^32
 * bytes); a 35,213 x 35,213 pair scoring 180,000.  Beyond those the planning,
 * packing and calibration code is checked on the CPU alone, for a subject of
 * 2^30 residues and queries of 2^24 rows (tests/native/length_check.cpp);
 * the kernels are not.                                                   */
SW_API int sw_db_create(sw_handle* h, const uint8_t* residues, const int64_t* offsets,
                 int64_t n, const int32_t* ids, sw_db** out);
SW_API int sw_db_free(sw_db* db);
SW_API int sw_db_get_stats(const sw_db* db, sw_db_stats* out);
/* Binary database file (the intent of the reference's
 * parse.py:40-46): subjects sorted by length (descending, stable) as encoded
 * codes + int64 offsets + int32 result ids, with an FNV-1a checksum, so a
 * database is parsed from FASTA once and then loaded in one read.  Loading
 * gives a database whose scans produce identical scores[id].            */
SW_API int sw_db_save(const sw_db* db, const char* path);
SW_API int sw_db_load(sw_handle* h, const char* path, sw_db** out);
/* Synthetic database generated in HBM: subject
 * k (k = 0..n-1, result id k) has global id id_base + k; its length is
 * len4096[h(seed, gid, "LENGTH") >> 52] and residue j is
 * lut65536[(h(seed, gid, j >> 2) >> 16 (j & 3)) & 0xffff], with
 * h(seed, id, k) = mix(seed * 0x9E3779B97F4A7C15 + mix(id * 0xD6E8FEB86659FD93
 * + k)) and mix = splitmix64's finaliser (all mod 2^64).  Lengths are
 * log-normal (median 290, sigma 0.657, [5, 35213]), residues Swiss-Prot
 * frequencies.  Only O(n) metadata is computed on the host; the residues
 * are written by device kernels (no host copy, no PCIe transfer).  Any
 * subject can be regenerated on a CPU from the two tables (sw_synth_tables)
 * and the formula above, e.g. to check sampled scores.                  */
SW_API int sw_db_create_synthetic(sw_handle* h, uint64_t seed, int64_t id_base, int64_t n,
                                  sw_db** out);
SW_API int sw_synth_tables(int32_t* len4096, uint8_t* lut65536);
SW_API int sw_synth_lengths(uint64_t seed, int64_t id_base, int64_t n, int32_t* lengths);
/* Per-subject lengths and result ids in the database's order (the order of
 * sw_db_create's input, or of the file for sw_db_load); either may be NULL. */
SW_API int sw_db_subjects(const sw_db* db, int64_t* lengths, int32_t* ids);
/* Subjects longer than `threshold` go to the intra-sequence kernel (one
 * wave per subject) instead of the inter-sequence kernels (one subject per
 * lane).  0 = library default: 5.7 x the mean length clamped to
 * [1024, 8192]; from 64,000 to 570,000 subjects (a rank's share of a strong-
 * scaled database) scaled by (n / 570,000)^0.4, floor 512; 64 for databases
 * under 64,000 subjects with a mean length >= 256 (too few 64-subject blocks
 * to fill the GPU).  May be changed between scans (re-packs the database). */
SW_API int sw_db_set_long_threshold(sw_db* db, int32_t threshold);
/* A database learns from the flagged counts its scans read back (without
 * waiting) which work to run in int16 first: the widest blocks and the long
 * subjects, per scoring and query length (sw_opts inter_i16_span and
 * intra_i16_first override it).  Scores never depend on that state; which
 * kernels a scan runs does.  This forgets it (and any readback in flight),
 * so the next scan runs as on a fresh database: a caller can time a cold
 * and a warm scan deliberately.                                            */
SW_API int sw_db_reset_adaptive(sw_db* db);

/* ---- scans ---------------------------------------------------------------
 * Replaces smith_waterman_cuda (SWSolver.cu:266-404): score the encoded
 * query against every subject; scores[id] = best local score.  The output
 * array must hold max(id)+1 int32; slots no subject maps to are set to 0.
 * Synchronous.                                                            */
SW_API int sw_scan(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
            const sw_scoring* sc, int32_t* scores_host);

/* Same, asynchronous on the handle's stream, scores written to DEVICE memory
 * (scores_dev; only slots that some subject maps to are written).  Used by
 * bench.py with the database already resident.  The handle must outlive the
 * database: sw_db_free uses the handle's stream.                          */
SW_API int sw_scan_device(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                   const sw_scoring* sc, int32_t* scores_dev);

/* Batch of nq queries (concatenated encoded residues, nq+1 offsets, query
 * k = queries[qoffsets[k] .. qoffsets[k+1])); scores_host is
 * [nq][max(id)+1].  The scans run back to back on the device with no host
 * synchronisation between queries (the reference's
 * main.cpp handles one query per run).  Synchronous.                      */
SW_API int sw_scan_batch(sw_handle* h, const sw_db* db, const uint8_t* queries,
                  const int64_t* qoffsets, int32_t nq, const sw_scoring* sc,
                  int32_t* scores_host);
/* Same, asynchronous on the handle's stream, into DEVICE memory scores_dev
 * [nq][max(id)+1] (only slots some subject maps to are written).          */
SW_API int sw_scan_batch_device(sw_handle* h, const sw_db* db, const uint8_t* queries,
                  const int64_t* qoffsets, int32_t nq, const sw_scoring* sc,
                  int32_t* scores_dev);

/* Timing of the most recent scan on this handle (waits for it). */
SW_API int sw_get_timing(sw_handle* h, sw_timing* out);
/* Kernel times summed over every scan since the last reset (waits for them);
 * *nscans = number of scans summed.  Lets a caller time many back-to-back
 * scans with HIP events on the stream they ran on, without synchronising
 * between them (bench.py).                                               */
SW_API int sw_timing_reset(sw_handle* h);
SW_API int sw_timing_total(sw_handle* h, sw_timing* out, int32_t* nscans);
/* Make another stream (hipStream_t, e.g. a top-K exchange stream) wait for
 * the handle's most recent scan to complete, through the scan's own end
 * event: no extra event record on the scan's stream (each is a packet the
 * command processor spends ~5 us on between two kernels).                 */
SW_API int sw_stream_wait_scan(sw_handle* h, void* hip_stream);
/* Name of the per-wave inter-sequence kernel the handle's last scan ran,
 * e.g. "sw_inter_x2<16,16,affine>" (packed int16, two subjects per lane) or
 * "sw_inter<32,8,affine>" (int32); "none" before any scan.  Valid until the
 * next scan on the handle.                                                  */
SW_API const char* sw_last_kernel(sw_handle* h);
/* Name of the intra-sequence (long-subject) kernel of the last scan:
 * "sw_intra_x2<16>" (two subjects per wave, packed fp16, with int32
 * re-scoring of flagged subjects), "sw_intra<6,affine>" (int32), or "none"
 * when the database has no long subjects.                                   */
SW_API const char* sw_last_intra_kernel(sw_handle* h);

/* ---- ranking ---------------------------------------------------------------
 * Top-k of a score vector (score descending, id ascending on ties).
 * Host-side helper for the multi-GPU top-K exchange.     */
SW_API int sw_topk(const int32_t* scores, int64_t n, int32_t k, int32_t* out_ids,
            int32_t* out_scores);

/* Device top-k, asynchronous on the handle's stream: the k best of
 * scores_dev[0..n) as int64 keys  score << 32 | (2^31 - 1 - (id_base + i)),
 * best first (score descending, id ascending); missing entries (n < k) are
 * INT64_MIN.  1 <= k <= 4096.  sw_topk_keys_device merges key vectors
 * (e.g. the all-gathered per-rank top-k of the multi-GPU exchange).        */
SW_API int sw_topk_device(sw_handle* h, const int32_t* scores_dev, int64_t n, int64_t id_base,
                   int32_t k, int64_t* keys_out_dev);
SW_API int sw_topk_keys_device(sw_handle* h, const int64_t* keys_dev, int64_t n, int32_t k,
                        int64_t* keys_out_dev);
/* A scan and its ranking in one synchronous call: the k best subjects of
 * the database for this query as int64 keys (sw_topk_device's: score << 32 |
 * 2^31 - 1 - result id, score descending, id ascending; INT64_MIN past the
 * database's end) in keys_host[k], from the device top-K over the scores of
 * every subject — only k keys cross PCIe.  The ranked output of main --topk
 * (the reference prints every score, main.cpp:58-60).  1 <= k <= 4096.    */
SW_API int sw_scan_topk(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                        const sw_scoring* sc, int32_t k, int64_t* keys_host);
/* Same as sw_topk_device with the global id of entry i read from
 * ids_dev[i] (device int32, >= 0) instead of id_base + i: a rank's
 * residue-balanced shard of one database holds scattered
 * global ids, and the merged ranking breaks ties by global id.            */
SW_API int sw_topk_device_ids(sw_handle* h, const int32_t* scores_dev, int64_t n, const int32_t* ids_dev,
                              int32_t k, int64_t* keys_out_dev);
/* A scan and the ranking of its scores, asynchronous on the handle's stream:
 * sw_scan_device into scores_dev, then keys_out_dev[k] = the k best subjects
 * of the database as sw_topk_device keys (score << 32 | 2^31 - 1 - global id,
 * best first, INT64_MIN past the database's end), over the subjects' result
 * ids r, with global id gid_dev[r] (device int32, >= 0) or, gid_dev NULL,
 * id_base + r: main.cpp:54-60's scan-then-collect for one shard of the
 * multi-GPU search in one call.  The top-K launch follows
 * every stage that writes the scores and precedes the scan's end event
 * (sw_stream_wait_scan).  1 <= k <= 4096.                                   */
SW_API int sw_scan_rank_device(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                               const sw_scoring* sc, int32_t* scores_dev, int32_t k, const int32_t* gid_dev,
                               int64_t id_base, int64_t* keys_out_dev);

/* ---- alignments of chosen hits (traceback) ------------------------------
 * The GPU analogue of the cpu.cpp pair program's traceback (cpu.cpp:47-108;
 * SURVEY.md §8 row f1): for each id in ids[0..n), the best local alignment of
 * the query against that database subject under cpu.cpp's rules — a cell
 * takes left, then up, then diagonal only on a strict improvement over 0,
 * the first strict maximum in row-major order is the end cell, and the walk
 * back stops at a zero cell.  Affine gaps (gap_open != gap_extend) use
 * this build's extension of those rules (the reference has no affine
 * traceback): a gap run opens unless extending is STRICTLY better, H takes
 * the run ending in the row (left), then the column (up), then the
 * diagonal, and the walk follows a run back to its opening cell; with
 * gap_open == gap_extend both give the same alignment.  Positions are
 * 1-based and inclusive; ops
 * (optional, n x ops_stride bytes, not NUL-terminated) spells the path from
 * the begin cell: 'M' an aligned pair, 'I' a query residue against a gap,
 * 'D' a subject residue against a gap; ops_len is the full path length even
 * when it exceeds ops_stride.  A slot shorter than its path holds the
 * path's first ops_stride ops, so it replays from (q_begin, s_begin); bytes
 * of a slot past min(ops_len, ops_stride) are unspecified.  ops == NULL:
 * positions and ops_len only.  Hits run in launches whose direction arrays
 * (one byte per cell) fit 1 GiB together (swplan::align_groups; a larger
 * single hit runs alone).  Cost O(|q| x |subject|) per hit: meant for the
 * top hits of a scan (e.g. the ids from sw_topk).                         */
typedef struct sw_alignment {
    int32_t score;
    int32_t q_begin, q_end;
    int32_t s_begin, s_end;
    int32_t ops_len;
} sw_alignment;
SW_API int sw_align(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                    const sw_scoring* sc, const int32_t* ids, int32_t n, sw_alignment* out,
                    char* ops, int64_t ops_stride);

/* ---- hit table: coordinates and statistics without a traceback ------------
 * One row per hit, what BLAST's tabular output or SSEARCH -m 8 prints (the
 * reference prints id:score only, main.cpp:58-60): where the alignment lies
 * in the query and in the subject, how long it is, its identities, positives
 * and gaps.  The alignment is the one sw_align reports, under the same tie
 * rules, linear and affine, and every field is a function of that
 * alignment's begin cell, end cell and ops string — but no direction matrix
 * is written and nothing is walked back: every column of the row is additive
 * along the path, so each DP value carries its path's begin cell and
 * counters forward (one wave per hit, memory O(|q| + |subject|), one pass).
 * The subjects are read from the resident packed database: only hit
 * descriptors go up and rows come down; a synthetic database regenerates
 * nothing on the host.
 *   sw_hit_stats : the rows of result ids[0..n), any n >= 0; an id the
 *                  database does not hold is SW_E_INVALID.
 *   sw_scan_hits : sw_scan_topk, then the rows of its ids in key order;
 *                  1 <= k <= 4096, *nhits = min(k, subjects).  Synchronous.
 * A hit of score 0, an empty subject or qlen == 0 reports 0 in every field
 * but id and s_len (sw_align's 1 / 0 begin / end pair is not carried over).
 * gap_opens counts maximal runs in the ops string, whatever the gap model
 * (under linear gaps every gap residue is a DP opening; the count does not
 * depend on that).  qlen + subject length < 2^31.  Arguments, error codes
 * and faults as sw_align.
 * Batches of queries (0.4.0; queries as in sw_scan_batch: concatenated codes
 * and nq+1 offsets), all synchronous, 1 <= k <= 4096, 0 <= n < 2^31:
 *   sw_scan_batch_topk : every query's device ranking, keys_host[nq][k] in
 *                  sw_topk_device's key form.  The scans run back to back,
 *                  each followed by its ranking, behind one score row: one
 *                  copy and one synchronisation per call, device memory
 *                  O(max_id + nq k).  An empty query ranks all-zero scores
 *                  (ids ascending); an empty database gives INT64_MIN keys;
 *                  nq == 0 writes nothing.
 *   sw_hit_stats_batch : the rows of the n pairs (query qidx[i], result id
 *                  ids[i]) into out[i], in the caller's order.  One launch
 *                  sequence mixes the queries, longest alignment first, and
 *                  every hit has its own scratch (two queries may hit one
 *                  subject).  A qidx outside [0, nq) or an id the database
 *                  does not hold is SW_E_INVALID.
 *   sw_scan_batch_hits : sw_scan_batch_topk, then the rows of every query's
 *                  ids in key order: out[nq][k] (stride k; rows past *nhits
 *                  are not written), *nhits = min(k, subjects), the same
 *                  for every query.  Two host synchronisations per call,
 *                  whatever nq is.
 * Out of scope: the PSSM forms, sw_group_*, and the ops string (that is
 * sw_align's job).  E-values and bit scores: the _sig forms below.        */
typedef struct sw_hit {
    int32_t id, score;
    int32_t q_begin, q_end, s_begin, s_end;   /* 1-based, inclusive, as sw_alignment */
    int32_t s_len;                            /* the subject's length (coverage) */
    int32_t length;                           /* alignment columns = sw_alignment.ops_len */
    int32_t identities;                       /* M columns whose two residue codes are equal */
    int32_t positives;                        /* M columns whose matrix entry is > 0 */
    int32_t gap_opens;                        /* maximal runs of I or of D in the path (ID = two) */
    int32_t gaps;                             /* I + D columns */
} sw_hit;
SW_API int sw_hit_stats(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                        const sw_scoring* sc, const int32_t* ids, int32_t n, sw_hit* out);
SW_API int sw_scan_hits(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                        const sw_scoring* sc, int32_t k, sw_hit* out, int32_t* nhits);
SW_API int sw_scan_batch_topk(sw_handle* h, const sw_db* db, const uint8_t* queries,
                              const int64_t* qoffsets, int32_t nq, const sw_scoring* sc,
                              int32_t k, int64_t* keys_host);
SW_API int sw_hit_stats_batch(sw_handle* h, const sw_db* db, const uint8_t* queries,
                              const int64_t* qoffsets, int32_t nq, const sw_scoring* sc,
                              const int32_t* qidx, const int32_t* ids, int64_t n, sw_hit* out);
SW_API int sw_scan_batch_hits(sw_handle* h, const sw_db* db, const uint8_t* queries,
                              const int64_t* qoffsets, int32_t nq, const sw_scoring* sc,
                              int32_t k, sw_hit* out, int32_t* nhits);

/* ---- E-values and bit scores: per-scan calibration (0.5.0) -----------------
 * The caller may pass any matrix, any gap pair and a PSSM, so no table of
 * Karlin-Altschul constants can serve; the significance of a hit is instead
 * calibrated on the scan's own scores, as SSEARCH does: regress the score on
 * ln(subject length) over the whole database, trim the related sequences,
 * and turn a hit's z-score into an extreme-value E-value.  The scores are in
 * HBM when the ranking runs: one more device pass counts them into a small
 * integer table that comes down beside the keys.
 *
 * Length bin of a subject of length L >= 1 (integer only): e = floor(log2 L),
 *   f = the two bits below L's leading bit ((L >> (e-2)) & 3 for e >= 2, else
 *   (L << (2-e)) & 3), b = 4e + f; L = 1, 2, 3, 4, 5, 7, 8 give 0, 4, 6, 8, 9,
 *   11, 12; b < 124.  The bin's abscissa is x_b = ln(2^e (1 + (f + 0.5)/4)).
 * Table uint32 hist[SW_CALIB_LBINS][SW_CALIB_SBINS]: every SUBJECT of the
 *   database (not every score slot) adds 1 at [b][min(max(score, 0), 511)]; a
 *   subject of length 0 is not counted.  Column 511 is the clip column and
 *   never enters the fit.  The table does not depend on the long threshold.
 * Fit (host, doubles) over the cells (b, s), s < 511, with weight hist[b][s]:
 *   weighted least squares of s on x_b gives the slope c and the intercept a;
 *   sigma^2 = sum w r^2 / (W - 2), r = s - a - c x_b.  Cells with |r / sigma|
 *   > 5 under the current a, c, sigma are dropped and the rest refitted, every
 *   cell being tested again under the LATEST fit, until the kept set does not
 *   change or 8 fits have run.  fits = regressions completed, n_fit = subjects
 *   in the last one, n_db = subjects counted, n_clipped = those in column 511.
 * Status bits:
 *   SW_CALIB_CLIPPED    the clip column holds more than 1 % of the counted
 *                       subjects (scores that grow with length: no local-
 *                       alignment statistic exists under such a scoring);
 *   SW_CALIB_FEW        fewer than 3 occupied length bins or fewer than 500
 *                       subjects were kept;
 *   SW_CALIB_DEGENERATE W < 3, fewer than two length bins (zero x-variance),
 *                       or sigma == 0: then c = 0, a = the kept scores' mean,
 *                       sigma = 0, every E-value is n_db and every bit score 0.
 * Significance of a hit of score s against a subject of length L (its own
 *   ln L, not its bin's):  z = (s - a - c ln L) / sigma,
 *   E = n_db (1 - exp(-exp(-(pi/sqrt 6) z - gamma)))  (through expm1),
 *   bits = ((pi/sqrt 6) z + gamma + ln(qlen L)) / ln 2,  gamma = Euler's constant.
 *   L = 0, a score <= 0 or qlen = 0 give E = n_db, bits = 0, z = 0.
 *
 *   sw_score_hist_device : the table of scores_dev (max_id + 1 slots, as a
 *                  scan wrote them) into hist_dev (device, 256 KB): a memset
 *                  and one kernel, asynchronous on the handle's stream.  The
 *                  per-subject length array it reads is uploaded on first use.
 *   sw_score_hist : the same into host memory; synchronous.
 *   sw_calib_fit, sw_calib_sig : the fit and the significance above; host
 *                  only, no handle.  sw_calib_fit sets n_skipped to 0 (a table
 *                  does not hold the zero-length subjects); the scan forms
 *                  below set it.
 *   sw_scan_hits_sig, sw_scan_batch_hits_sig : sw_scan_hits and
 *                  sw_scan_batch_hits with sig[i] = sw_calib_sig(calib, row i's
 *                  score, row i's s_len) beside every row and the scan's
 *                  calibration in *calib (calib[nq], sig[nq][k] for the batch;
 *                  calib may be NULL).  The table's launch follows every stage
 *                  that writes that query's scores, its rescue tail included,
 *                  and precedes the next query's scan; the tables come down
 *                  with the keys: the batch keeps its two host synchronisations.
 *   sw_scan_pssm_topk_calib : sw_scan_pssm_topk and the scan's calibration
 *                  (there is no PSSM hit table: the caller applies sw_calib_sig
 *                  to the keys' scores and sw_db_subjects' lengths).
 * Out of scope: sw_group_*, composition-based score adjustment, and a search
 * space other than the database scanned (n_db is its subject count).        */
#define SW_CALIB_LBINS 128
#define SW_CALIB_SBINS 512
#define SW_CALIB_CLIPPED 1
#define SW_CALIB_FEW 2
#define SW_CALIB_DEGENERATE 4
typedef struct sw_calib {
    int32_t size;        /* sizeof(sw_calib), set by sw_calib_fit (ABI check) */
    int32_t status;      /* SW_CALIB_* bits */
    int32_t qlen;        /* the query's length (the bit score's search space) */
    int32_t fits;        /* regressions completed (0: degenerate at once) */
    int64_t n_db;        /* subjects counted */
    int64_t n_fit;       /* subjects in the last fit */
    int64_t n_clipped;   /* subjects in the clip column */
    int64_t n_skipped;   /* zero-length subjects (not counted) */
    double a, c, sigma;  /* score = a + c ln L, residual standard deviation */
} sw_calib;
typedef struct sw_sig {
    double evalue, bits, z;
} sw_sig;
SW_API int sw_score_hist_device(sw_handle* h, const sw_db* db, const int32_t* scores_dev, uint32_t* hist_dev);
SW_API int sw_score_hist(sw_handle* h, const sw_db* db, const int32_t* scores_dev, uint32_t* hist_host);
SW_API int sw_calib_fit(const uint32_t* hist, int32_t qlen, sw_calib* out);
SW_API int sw_calib_sig(const sw_calib* calib, int32_t score, int32_t slen, sw_sig* out);
SW_API int sw_scan_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                            const sw_scoring* sc, int32_t k, sw_hit* out, sw_sig* sig, int32_t* nhits,
                            sw_calib* calib);
SW_API int sw_scan_batch_hits_sig(sw_handle* h, const sw_db* db, const uint8_t* queries,
                                  const int64_t* qoffsets, int32_t nq, const sw_scoring* sc, int32_t k,
                                  sw_hit* out, sw_sig* sig, int32_t* nhits, sw_calib* calib);

/* ---- ranking by E-value, with an E-value cutoff (0.6.0) -------------------
 * The _sig forms above rank by raw score and attach the significance to what
 * came out; the statistic is length-regressed (z = (s - a - c ln L) / sigma),
 * so their rows are not in E-value order and a short significant subject just
 * under the k-th raw score is absent.  The _ranked forms rank by the statistic
 * itself, as SSEARCH does, and take a threshold ("all hits with E <= 10").
 * The step between the fit and the ranking is one more device pass over every
 * subject.  The ranking is defined on integers, so host, device and tests
 * agree bit for bit:
 *   adj[L]   = llround(4096 c ln L) for L >= 1, adj[0] = 0, saturated to int32;
 *              all zero when the calibration is DEGENERATE (sw_sig_rank_table).
 *   r(s, L)  = clamp(s, 0, 2^20 - 1) * 4096 - adj[min(L, max_len)], saturated
 *              to [SW_RANK_FLOOR, 2^32 - 1], SW_RANK_FLOOR = -2^32 + 1; a subject
 *              with s <= 0 or L = 0 has r = SW_RANK_FLOOR (its E is n_db).
 *              Ranking by r is ranking by z at 1/4096 of a score unit.
 *   key      = r * 2^31 + (2^31 - 1 - id): r descending, then id ascending;
 *              INT64_MIN = absent (past the database's end, or cut off).  The
 *              keys go through sw_topk_keys_device's selection unchanged.
 *   cutoff   : a subject passes iff r >= r_min, r_min = ceil(4096 (a + sigma
 *              z_min)) with z_min solving E(z_min) = max_evalue in the E-value
 *              formula above (sw_sig_rank_min).  max_evalue >= n_db or +inf:
 *              SW_RANK_FLOOR (no cutoff).  DEGENERATE: SW_RANK_FLOOR if
 *              max_evalue >= n_db, else 2^32 (nothing passes).  max_evalue <= 0
 *              or NaN: SW_E_INVALID.  The cutoff is applied to the KEY: a
 *              reported E-value (the exact double of sw_calib_sig) can sit a
 *              relative 1e-4 either side of max_evalue at the edge.
 *
 *   sw_sig_rank_table, sw_sig_rank_min : host only, no handle; adj holds
 *                  max_len + 1 entries.
 *   sw_sig_topk_device : asynchronous on the handle's stream: uploads
 *                  adj_host[0 .. max_len] (it must stay valid until the stream
 *                  has passed the call's work), zeroes *count_out_dev, writes
 *                  every subject's key (INT64_MIN below r_min) into the handle's
 *                  workspace while counting the subjects that pass, exactly,
 *                  into *count_out_dev (device uint32), then selects the k best
 *                  keys, best first, into keys_out_dev[k] (INT64_MIN past the
 *                  last passing subject).  scores_dev holds max_id + 1 slots as
 *                  a scan wrote them; a slot no subject maps to is never read.
 *                  1 <= k <= 4096.
 *   sw_scan_hits_ranked, sw_scan_batch_hits_ranked : the scan and its table,
 *                  the fit (first synchronisation), the key pass and selection
 *                  (second), the hit-table rows of the selected ids (third).
 *                  *nhits = min(k, *n_pass) rows in key order (out[nq][k],
 *                  sig[nq][k], nhits[nq], n_pass[nq], calib[nq] for the batch;
 *                  calib may be NULL), sig[i] = sw_calib_sig(calib, row i's
 *                  score, row i's s_len); *n_pass, the subjects that pass the
 *                  cutoff, may exceed k: the list was truncated.  max_evalue
 *                  +inf: no cutoff.  An empty database gives 0 and 0.  The fit
 *                  must precede the ranking, so a batch cannot share one score
 *                  row: it keeps G = max(1, min(nq, score_bytes / (4 slots)))
 *                  rows (slots = max_id + 1; score_bytes 0 = 256 MiB) and runs
 *                  groups of G queries, each group's scans and tables, one
 *                  synchronisation, its fits, key passes and selections; then
 *                  one synchronisation and every query's rows in one launch
 *                  sequence: three synchronisations when the rows fit.
 *   sw_scan_pssm_topk_ranked : the same for a PSSM; there is no PSSM hit table,
 *                  so a device gather writes ids[i], scores[i] and the
 *                  significance comes from the subject's length; two
 *                  synchronisations.
 * Out of scope: sw_group_*, composition-based score adjustment, a PSSM hit
 * table.                                                                     */
#define SW_RANK_SCALE 4096
#define SW_RANK_FLOOR (-4294967295LL)   /* -2^32 + 1 */
#define SW_RANK_NONE 4294967296LL       /* 2^32: an r_min nothing passes */
SW_API int sw_sig_rank_table(const sw_calib* calib, int32_t max_len, int32_t* adj);
SW_API int sw_sig_rank_min(const sw_calib* calib, double max_evalue, int64_t* r_min);
SW_API int sw_sig_topk_device(sw_handle* h, const sw_db* db, const int32_t* scores_dev, const int32_t* adj_host,
                              int32_t max_len, int64_t r_min, int32_t k, int64_t* keys_out_dev,
                              uint32_t* count_out_dev);
SW_API int sw_scan_hits_ranked(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen,
                               const sw_scoring* sc, int32_t k, double max_evalue, sw_hit* out, sw_sig* sig,
                               int32_t* nhits, int64_t* n_pass, sw_calib* calib);
SW_API int sw_scan_batch_hits_ranked(sw_handle* h, const sw_db* db, const uint8_t* queries,
                                     const int64_t* qoffsets, int32_t nq, const sw_scoring* sc, int32_t k,
                                     double max_evalue, int64_t score_bytes, sw_hit* out, sw_sig* sig,
                                     int32_t* nhits, int64_t* n_pass, sw_calib* calib);

/* ---- profile (PSSM) queries ------------------------------------------------
 * A position-specific scoring matrix in the place of a query: a [qlen][25]
 * int8 table, rows[i*25 + c] = score of subject residue code c at query
 * position i (a PSI-BLAST checkpoint, a family profile; the reference scores
 * residues against one 25 x 25 table only, SWSolver.cu:54-81).  Every scan
 * kernel reads a per-query profile already; a PSSM only changes what that
 * profile is built from, so every kernel family, the guard bands, the ranking
 * and the traceback serve it unchanged, and the table derived from a sequence
 * and a matrix (rows[i] = matrix[q[i]]) scans bit for bit as sw_scan does.
 *   sw_pssm_create : validates the entries (-100..100) and qlen >= 0, uploads
 *                    the table once, asynchronously on the handle's stream
 *                    (rows may be freed on return); qlen == 0 is valid and
 *                    scans to all zeros, as the empty query does.
 *   sw_pssm_free   : waits for the handle's stream (scans in flight read the
 *                    table); the handle must outlive the PSSM.
 *   sw_scan_pssm, sw_scan_pssm_device, sw_scan_pssm_topk, sw_align_pssm :
 *                    as sw_scan, sw_scan_device, sw_scan_topk and sw_align,
 *                    with the gap model given as two integers (1..1000;
 *                    equal = linear).  A PSSM scan copies nothing from the
 *                    host.  A PSSM of another handle's device is SW_E_INVALID.
 * Out of scope: batches of PSSMs, the sw_group_* forms, sw_score_pair and
 * position-specific gap costs.  Building a PSSM from hits: "iterated profile
 * search" below.                                                            */
typedef struct sw_pssm sw_pssm;
SW_API int sw_pssm_create(sw_handle* h, const int8_t* rows, int32_t qlen, sw_pssm** out);
SW_API int sw_pssm_free(sw_pssm* p);
SW_API int sw_pssm_length(const sw_pssm* p, int32_t* qlen);
SW_API int sw_scan_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                        int32_t gap_extend, int32_t* scores_host);
SW_API int sw_scan_pssm_device(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                               int32_t gap_extend, int32_t* scores_dev);
SW_API int sw_scan_pssm_topk(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                             int32_t gap_extend, int32_t k, int64_t* keys_host);
SW_API int sw_align_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                         int32_t gap_extend, const int32_t* ids, int32_t n, sw_alignment* out,
                         char* ops, int64_t ops_stride);
/* sw_scan_pssm_topk and the scan's calibration (see "E-values and bit scores"). */
SW_API int sw_scan_pssm_topk_calib(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                                   int32_t gap_extend, int32_t k, int64_t* keys_host, sw_calib* calib);
/* A PSSM scan ranked by E-value (see "ranking by E-value"): ids[k], scores[k],
 * sig[k], of which the first *nhits = min(k, *n_pass) are written. */
SW_API int sw_scan_pssm_topk_ranked(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open,
                                    int32_t gap_extend, int32_t k, double max_evalue, int32_t* ids,
                                    int32_t* scores, sw_sig* sig, int32_t* nhits, int64_t* n_pass,
                                    sw_calib* calib);

/* ---- iterated profile search: a PSSM built from a scan's hits (0.7.0) ------
 * The step from SSEARCH to PSI-BLAST: the subjects a calibrated E-value
 * includes are aligned against the current profile, their alignments make a
 * query-anchored multiple alignment, and its weighted residue counts, mixed
 * with matrix-derived pseudocounts, are the next profile.  The rows and the
 * counts are built on the device (the subjects' residues and the direction
 * arrays are there; only small integer tables come down); the step from
 * tables to scores is host arithmetic in doubles.
 *
 * Rows.  For n hits against a PSSM of qlen positions, msa[(n+1)][qlen] bytes:
 *   row 0 is the master sequence (the query's codes), or all SW_MSA_NONE when
 *   none is given; row 1+k is the alignment sw_align_pssm reports for ids[k]:
 *   position i holds the subject's residue code under an 'M', SW_MSA_GAP under
 *   an 'I' ('D' columns have no query position), and SW_MSA_NONE outside
 *   [q_begin, q_end].  A hit of score 0 or an empty subject is an all-NONE row.
 *   The walk back writes the row itself: no ops slot can truncate it.
 * Tables (integers only: host, device and tests agree bit for bit).  Only the
 *   codes 0..19 are counted; 20..24, GAP and NONE never are.
 *   cnt[i][a]  uint32 [qlen][20]: rows r with msa[r][i] == a;
 *   k_i        codes a with cnt[i][a] > 0;
 *   term(i,a)  = floor(SW_PROFILE_ONE / (k_i cnt[i][a])): Henikoff position-
 *              based weights in fixed point, SW_PROFILE_ONE = 2^30;
 *   weight[r]  uint64 [n+1]: floor(u_r / cov_r), u_r the sum of
 *              term(i, msa[r][i]) over the cov_r columns where row r holds a
 *              counted code; 0 when cov_r is 0;
 *   wsum[i][a] uint64 [qlen][20]: the sum of weight[r] over the rows with
 *              msa[r][i] == a (below 2^43).
 * From tables to a PSSM (host).  p_a: the Swiss-Prot composition the synthetic
 *   generator draws from, normalised.  lambda: the positive root of
 *   sum_{a,b<20} p_a p_b exp(lambda s[a][b]) = 1, by bisection in doubles; it
 *   exists iff the expected score is negative and some entry is positive
 *   (else SW_E_UNSUPPORTED).  For a position with T_i = sum_a wsum[i][a] > 0:
 *   f_i(a) = wsum[i][a] / T_i, alpha = k_i - 1, beta = pseudo (in (0, 1000];
 *   10 is the usual value), g_i(a) = p_a sum_b f_i(b) exp(lambda s[b][a]) (row:
 *   the query-side code), Q_i(a) = (alpha f_i(a) + beta g_i(a)) / (alpha + beta),
 *   rows[i][a] = clamp(llround(ln(Q_i(a) / p_a) / lambda), -100, 100) for
 *   a < 20; columns 20..24 are the prior table's.  T_i = 0: the whole prior
 *   row.  One observed residue: alpha = 0 and the row is the matrix's row for
 *   it.  Scores stay on the matrix's scale, so the gap costs keep their meaning.
 *
 *   sw_pssm_rows   : the [qlen][25] table a PSSM was created from.
 *   sw_msa_pssm    : the rows into host memory (msa_host[(n+1)][qlen]); al
 *                    (nullable, [n]): the alignments' coordinates too.
 *   sw_profile_counts : the rows and the three tables on the device; only the
 *                    tables come down (each may be NULL).
 *   sw_profile_counts_msa : the tables of rows the caller uploads
 *                    (msa_host[nrows][qlen], 1 <= nrows <= 4097, any byte
 *                    values): the kernels' own entry point.
 *   sw_matrix_lambda, sw_pssm_from_counts : host only, no handle; matrix NULL:
 *                    SW_MATRIX_BLOSUM50_REF; rows_out may alias prior_rows.
 *   sw_pssm_refine : sw_profile_counts, sw_pssm_from_counts with the PSSM's own
 *                    rows as the prior, sw_pssm_create.
 *   sw_search_iter : P_1 is the table derived from the query (rows[i] =
 *                    matrix[q[i]]).  Round t: one scan of P_t and its
 *                    calibration, then a key pass and a selection with
 *                    max_evalue = inclusion_evalue and k = include_max
 *                    (1..4096): the selected ids are the included set I_t.
 *                    Stop when t = rounds (>= 1) or I_t = I_{t-1} as sets
 *                    (*converged = 1); else P_{t+1} = refine(P_t, I_t, master =
 *                    the query).  The report (ids, scores, sig: the first
 *                    *nhits = min(k, *n_pass) of [k]; calib, nullable) is a
 *                    second key pass and selection over the LAST round's scores
 *                    with (k, max_evalue), not another scan.  rounds_log
 *                    (nullable, [rounds]): per round run, the included, added
 *                    and dropped counts and that round's calibration;
 *                    *rounds_run of them are written.  final_pssm (nullable):
 *                    the last round's profile, the caller's to free.
 *                    Edges: the included, reported and fed-back ids are RESULT
 *                    ids (whatever ids the database was created with).  A
 *                    round that includes nothing still refines (n = 0, the
 *                    master alone: columns 0..19 of a row become the matrix's
 *                    for the query's residue, columns 20..24 and the rows
 *                    where the query holds a code 20..24 stay the prior's, so
 *                    P_2 = P_1), and the next round converges on the empty
 *                    set; so do an empty
 *                    database (*nhits = 0) and qlen = 0 (every score 0; the
 *                    report under no cutoff is then the k lowest ids).
 *                    rounds = 1 never refines and needs no lambda; rounds > 1
 *                    under a matrix without one is SW_E_UNSUPPORTED before
 *                    any scan.
 * n is 0..4096; ids may repeat; an id the database does not hold is
 * SW_E_INVALID.  The hits run in swplan::align_groups' launch groups.  All
 * synchronous.  sw_align and sw_align_pssm are unchanged.
 * Out of scope: a PSSM hit table, sw_group_*, purging near-identical rows,
 * gaps as a 21st letter, composition-based adjustment, position-specific gap
 * costs, batches of queries.                                               */
#define SW_MSA_GAP 25
#define SW_MSA_NONE 26
#define SW_PROFILE_CODES 20
#define SW_PROFILE_ONE 1073741824   /* 2^30 */
#define SW_PROFILE_MAX_HITS 4096
typedef struct sw_iter_round {
    int32_t included;    /* |I_t| */
    int32_t added;       /* |I_t \ I_{t-1}| (I_0 is empty) */
    int32_t dropped;     /* |I_{t-1} \ I_t| */
    int32_t reserved;
    sw_calib calib;      /* round t's calibration */
} sw_iter_round;
SW_API int sw_pssm_rows(const sw_pssm* p, int8_t* rows);
SW_API int sw_msa_pssm(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                       const uint8_t* master, const int32_t* ids, int32_t n, uint8_t* msa_host, sw_alignment* al);
SW_API int sw_profile_counts(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                             const uint8_t* master, const int32_t* ids, int32_t n, uint32_t* cnt, uint64_t* weight,
                             uint64_t* wsum);
SW_API int sw_profile_counts_msa(sw_handle* h, const uint8_t* msa_host, int32_t nrows, int32_t qlen, uint32_t* cnt,
                                 uint64_t* weight, uint64_t* wsum);
SW_API int sw_matrix_lambda(const int8_t* matrix, double* lambda);
SW_API int sw_pssm_from_counts(const uint32_t* cnt, const uint64_t* wsum, int32_t qlen, const int8_t* prior_rows,
                               const int8_t* matrix, double pseudo, int8_t* rows_out);
SW_API int sw_pssm_refine(sw_handle* h, const sw_db* db, const sw_pssm* p, int32_t gap_open, int32_t gap_extend,
                          const uint8_t* master, const int8_t* matrix, double pseudo, const int32_t* ids, int32_t n,
                          sw_pssm** out);
SW_API int sw_search_iter(sw_handle* h, const sw_db* db, const uint8_t* query, int32_t qlen, const sw_scoring* sc,
                          int32_t rounds, double inclusion_evalue, int32_t include_max, double pseudo, int32_t k,
                          double max_evalue, int32_t* ids, int32_t* scores, sw_sig* sig, int32_t* nhits,
                          int64_t* n_pass, sw_calib* calib, sw_iter_round* rounds_log, int32_t* rounds_run,
                          int32_t* converged, sw_pssm** final_pssm);

/* ---- single pair ---------------------------------------------------------
 * One query against one subject on the GPU (wavefront kernel); the GPU
 * analogue of the cpu.cpp pair program's score (cpu.cpp:43-74).         */
SW_API int sw_score_pair(sw_handle* h, const uint8_t* query, int32_t qlen,
                  const uint8_t* subject, int32_t slen, const sw_scoring* sc,
                  int32_t* score);

/* ---- several GPUs of one process -------------------------
 * Replaces the reference's single-GPU scan loop (main.cpp:54-56 ->
 * smith_waterman_cuda, SWSolver.cu:266-404) with one database sharded over
 * the devices of a group.  sw_group_create: one handle per listed device.
 * The first sw_group_topk of a group of DISTINCT devices creates an RCCL
 * communicator over them (ncclCommInitAll; librccl is loaded at run time,
 * only then: sw_group_scan needs no collective and no RCCL).  A device listed
 * twice is allowed (one-GPU tests), and RCCL that cannot be loaded or
 * initialised is tolerated: the top-K exchange then goes through the host.
 * sw_group_db_create: LPT shards over subject lengths (longest first, each to
 * the lightest shard, lowest index on ties: residue-balanced and
 * deterministic), one resident sw_db per device, built in parallel.
 * sw_group_scan: scores_host[id] of every subject (as sw_scan), the devices
 * scanning concurrently (one host thread each).  sw_group_topk: the k best
 * (score desc, id asc) as sw_topk_device keys in keys_host[k]: per-device
 * top-k with global ids, ONE ncclAllGather of k int64 keys per device, merge
 * on device 0.  All synchronous.                                          */
typedef struct sw_group sw_group;
typedef struct sw_gdb sw_gdb;
SW_API int sw_group_create(const int32_t* devices, int32_t ndev, sw_group** out);
SW_API int sw_group_destroy(sw_group* g);
/* The top-K exchange path: "rccl allgather (N ranks)" once the communicators
 * exist, "rccl allgather (communicators created by the first top-K)" before,
 * or "host (<why>)". */
SW_API const char* sw_group_info(const sw_group* g);
/* The handle of device slot d (owned by the group). */
SW_API int sw_group_handle(sw_group* g, int32_t d, sw_handle** out);
SW_API int sw_group_db_create(sw_group* g, const uint8_t* residues, const int64_t* offsets, int64_t n,
                              const int32_t* ids, sw_gdb** out);
SW_API int sw_group_db_free(sw_gdb* gdb);
/* Subjects and residues of shard d. */
SW_API int sw_group_db_shard(const sw_gdb* gdb, int32_t d, int64_t* n_subjects, int64_t* residues);
SW_API int sw_group_scan(sw_group* g, const sw_gdb* gdb, const uint8_t* query, int32_t qlen,
                         const sw_scoring* sc, int32_t* scores_host);
SW_API int sw_group_topk(sw_group* g, const sw_gdb* gdb, const uint8_t* query, int32_t qlen,
                         const sw_scoring* sc, int32_t k, int64_t* keys_host);

#ifdef __cplusplus
}
#endif
#endif /* SW_AMD_H */
