/*
 * cropsr_hip.h -- C ABI of libcropsr_hip.so, the MI355X (gfx950) PAM-scan +
 * on-target-score engine that replaces CROPSR's inner loop.
 *
 * The reference (H2muller/CROPSR) is one Python script and has no FFI of its
 * own; the two seams this library slots into are
 *
 *   seam 1  CROPSR.py:413-434  per contig string: regex (?=.GG) / (?=CC.) scan,
 *           window slicing and keep-filter that append to Complete_dataset
 *           -> crp_arena_* + crp_scan_score + crp_fetch_hits
 *   seam 2  CROPSR.py:285-313, called at :461  rs1_score(ndarray[n,30] uint8)
 *           -> ndarray[n] float64      -> crp_score_30mers
 *   seam 3  (opt-in) CROPSR.py:77-95 parses the GFF, :375 drops the table, :466-468 write '' into `features`: the join
 *           those lines stop short of -> crp_annotation_build / _track (host) + crp_annotate_set_track / _lookup (GPU)
 *
 * The binding a CROPSR maintainer would add (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns 0 (CRP_OK) or a negative
 *     crp_status; nothing throws, aborts or prints.
 *   - the caller owns every host buffer; the library owns every device buffer.
 *   - one crp_ctx per GPU; calls on one handle are serialised by the caller.  Two ways to the whole node: one
 *     process per GPU, each with its own crp_ctx and an RCCL communicator across them (crp_comm_*), or ONE process
 *     with a crp_node over N devices (crp_node_*: the fan-out, the cut of the genome and the gatherv happen inside
 *     the library) -- what the single-process reference script binds.
 *   - there is NO CPU fallback: without a usable HIP device crp_init fails.
 *
 * Coordinates.  A contig is handed over as the exact character string the
 * reference scans (CROPSR.py:409 `sequence`, including the decoration left by
 * cropsr_functions.py:221-229 when the FASTA was re-formatted), one byte per
 * character.  Hit positions come back as indices into that string:
 *   '+' table: i = re match index of (?=.GG)   start_pos=i-l end_pos=i cutsite=i-3
 *   '-' table: j = re match index of (?=CC.)   start_pos=j+3+l end_pos=j+3 cutsite=j
 * shifted by the contig's arena offset (see crp_arena_add_contig_*).
 */
#ifndef CROPSR_HIP_H
#define CROPSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRP_ABI_VERSION 6

typedef enum crp_status {
    CRP_OK = 0,
    CRP_ERR_INVALID = -1,     /* bad argument */
    CRP_ERR_NO_DEVICE = -2,   /* no usable HIP device: none, or not a gfx950 (never falls back to CPU) */
    CRP_ERR_HIP = -3,         /* a HIP runtime call failed; see crp_last_error */
    CRP_ERR_NOMEM = -4,       /* host or device allocation failed */
    CRP_ERR_STATE = -5,       /* call out of order (e.g. scan before seal) */
    CRP_ERR_CAPACITY = -6,    /* arena capacity exceeded */
    CRP_ERR_UNSUPPORTED = -7, /* e.g. guide length outside [0, 50] */
    CRP_ERR_IO = -8,          /* write(2) on the caller's descriptor failed; errno is left set */
    CRP_ERR_COMM = -9,        /* an RCCL call failed or librccl.so could not be loaded; see crp_last_error */
    CRP_ERR_PEER = -10        /* a collective call was abandoned ON EVERY RANK because another rank reported an error
                               * before the exchange started (crp_gather_hits); this rank itself was fine */
} crp_status;

typedef struct crp_ctx crp_ctx;
typedef struct crp_arena crp_arena;

/* ---- library ----------------------------------------------------------- */
int crp_abi_version(void);
const char *crp_strerror(int status);

/* ---- context ----------------------------------------------------------- */
/* Opens HIP device `device_id` (index as seen by this process). */
int crp_init(int device_id, crp_ctx **out);
int crp_destroy(crp_ctx *ctx);
/* Text of the last failing HIP call on this context ("" if none). */
const char *crp_last_error(const crp_ctx *ctx);
/* Name / CU count / HBM bytes of the device, for logs and bench output. */
int crp_device_info(const crp_ctx *ctx, char *name, int name_cap, int *n_cu, uint64_t *hbm_bytes);

/* ---- host-side packing (no GPU needed) --------------------------------- */
/* Number of 64-base words one contig of `len` characters occupies in an arena
 * (its bases, padded to a word, plus one separator word). */
uint64_t crp_arena_words_for(uint64_t len);
/* Arena words needed for contigs whose crp_arena_words_for() sum is `sum`
 * (adds the leading and trailing separator words). */
uint64_t crp_arena_words_total(uint64_t sum);
/* Largest capacity_words crp_arena_create accepts (arena positions stay below 2^31);
 * a bigger genome is spread over several arenas, contig by contig. */
uint64_t crp_arena_max_words(void);
/* Classify `len` characters into the four bit-planes the kernels read, 64
 * characters per word, bit k of word w = character 64*w + k:
 *   hi,lo  2-bit base code, alphabet order of CROPSR.py:300 (A=00 T=01 C=10 G=11)
 *   up     upper-case base: complemented on the '+' strand (CROPSR.py:128 only
 *          maps upper case) and eligible for the PAM (regexes match 'G'/'C' only)
 *   ac     a scoring base (acgtACGT; 'U' counts as 'A')
 * Characters past `len` in the last word are encoded as "void" (outside any
 * contig).  Each plane needs ceil(len/64) words.  n_threads <= 1: serial. */
int crp_pack_ascii(const uint8_t *text, uint64_t len, uint64_t *hi, uint64_t *lo,
                   uint64_t *up, uint64_t *ac, int n_threads);

/* ---- arena: the device-resident genome --------------------------------- */
/* An arena holds any number of contigs as four bit-planes in HBM, separated by
 * void words, so one kernel launch scans all of them.  capacity_words bounds
 * the total (use crp_arena_words_total). */
int crp_arena_create(crp_ctx *ctx, uint64_t capacity_words, crp_arena **out);
int crp_arena_destroy(crp_arena *arena);
/* Append one contig given as characters; packing runs on the GPU.  Returns the
 * arena offset (in characters) of its first character: a hit at arena position
 * P belongs to the contig with the largest offset <= P, at index P - offset. */
int crp_arena_add_contig_ascii(crp_arena *arena, const uint8_t *text, uint64_t len,
                               uint64_t *arena_offset);
/* n contigs in one call, in order (arena_offsets: n values, may be NULL).  Same result as n calls of
 * crp_arena_add_contig_ascii; small contigs (an assembly's scaffolds) share one host-to-device copy and one pack
 * launch per ~31 MiB instead of paying a copy, a launch and an event each.  On an error the contigs before the failing
 * one have been added. */
int crp_arena_add_contigs_ascii(crp_arena *arena, const uint8_t *const *texts, const uint64_t *lens, uint64_t n,
                                uint64_t *arena_offsets);
/* Same, from planes packed on the host with crp_pack_ascii. */
int crp_arena_add_contig_packed(crp_arena *arena, const uint64_t *hi, const uint64_t *lo,
                                const uint64_t *up, const uint64_t *ac, uint64_t len,
                                uint64_t *arena_offset);
/* No more contigs; waits for the uploads. */
int crp_arena_seal(crp_arena *arena);
/* The tile shape the arena was sealed with (1 LARGE, 2 SMALL: CRP_OPT_TILE_GEOMETRY), its number of tiles
 * (= workgroups per scan) and the words of one tile.  Any pointer may be NULL. */
int crp_arena_tiles(const crp_arena *arena, int *geometry, uint64_t *n_tiles, uint64_t *tile_words);
/* Totals: contigs, characters, words used. */
int crp_arena_stats(const crp_arena *arena, uint64_t *n_contigs, uint64_t *n_chars, uint64_t *n_words);

/* What the arena's characters are, counted on the GPU from the planes: upper-case A/C/G/T, and everything else
 * (lower case, N, IUPAC codes, the decoration characters of cropsr_functions.py:221-229).  An arena whose n_other is
 * nothing but decoration (<= 4 per contig) is the "entirely upper-case ACGT" input for which SURVEY.md 8(d) leaves the
 * two 1-bit planes out of the algorithmic bytes (bench.py).  Either pointer may be NULL. */
int crp_arena_composition(crp_arena *arena, uint64_t *n_plain, uint64_t *n_other);

/* ---- seam 1 + 2 over a whole arena -------------------------------------- */
/* Scan both strands of every contig, keep what CROPSR.py:419/:430 keep for
 * guide length `guide_len` (0..50; the reference takes any integer: for lengths outside that range scan with the
 * nearer end of it -- a superset of the reference's hits, none of them scored at those lengths -- and apply
 * CROPSR.py:419/:430 to the positions on the host, as cropsr_amd/cli.py refilter_hits does), score every kept hit whose long_sequence has exactly
 * 30 characters (guide_len == 20: complete windows; > 20: only windows the end of
 * the string cuts to 30; < 20: none -- the others get -1 like CROPSR.py:466-468), leave
 * the tables in HBM.  Tables are ascending in arena position per strand, i.e.
 * per contig in the reference's own order.  flags: CRP_SCAN_PRE also keeps the
 * pre-sigmoid sum (CROPSR.py:312). */
#define CRP_SCAN_PRE 1    /* (flags == 1 is what callers of ABI version 2 passed as `want_pre`) */
/* CRP_SCAN_SEEDS: the scan also writes, per kept hit, the 12 characters of `sequence` next to the PAM that the
 * off-target seed scan (below) works on -- the emit kernel holds every hit's window in registers anyway.
 * crp_offtarget_add then takes them from there instead of reading the planes a second time.  Honoured for
 * guide_len == 20; for other lengths the flag is ignored and crp_offtarget_add derives the seeds itself. */
#define CRP_SCAN_SEEDS 2
int crp_scan_score(crp_arena *arena, int guide_len, int flags,
                   uint64_t *n_plus, uint64_t *n_minus);
/* Copy the tables of the last crp_scan_score to host arrays sized n_plus /
 * n_minus.  Any pointer may be NULL to skip that column. */
int crp_fetch_hits(crp_arena *arena, uint32_t *pos_plus, double *pre_plus, double *score_plus,
                   uint32_t *pos_minus, double *pre_minus, double *score_minus);
/* Rows of the '+' and '-' tables of the last crp_scan_score (what it returned in *n_plus / *n_minus). */
int crp_hits_counts(const crp_arena *arena, uint64_t *n_plus, uint64_t *n_minus);
/* Device addresses of the same tables (valid until the next crp_scan_score or
 * crp_arena_destroy) for a device-to-device gather such as RCCL send/recv. */
int crp_hits_device(crp_arena *arena, void **pos_plus, void **score_plus,
                    void **pos_minus, void **score_minus);

/* ---- seam 2 alone -------------------------------------------------------- */
/* Floating-point accumulation order of the two matmuls inside rs1_score
 * (CROPSR.py:305,311).  With the reference's BLAS the order a row is summed in
 * depends on its place in the batch of n rows handed to rs1_score:
 *   BODY4  rows 0 .. 4*floor(n/4)-1, and the last row if n%4 is 1 or 3
 *   TAIL2  rows 4*floor(n/4) and 4*floor(n/4)+1 if n%4 is 2 or 3
 *   DOT1   the single row of a batch with n == 1
 * crp_scan_score always uses BODY4; a host that wants the reference's CSV bytes
 * re-scores the <= 2 TAIL2 rows (or the DOT1 row) of each written chunk. */
#define CRP_ORDER_BODY4 0
#define CRP_ORDER_TAIL2 1
#define CRP_ORDER_DOT1 2
/* rs1_score (CROPSR.py:285-313) on n rows of 30 bytes, row-major, exactly the
 * array CROPSR.py:458-461 builds: bytes equal to 'A','T','C','G' select weights,
 * every other byte selects none.  Every row is summed in `order`.  pre may be
 * NULL. */
int crp_score_30mers(crp_ctx *ctx, const uint8_t *rows, uint64_t n, int order, double *pre, double *score);

/* ---- output side: native CSV rows (host code, no GPU needed) ---------------- */
/* Formats n_rows rows of ONE contig exactly as the reference's row tuples go through
 * csv.writer.writerows (CROPSR.py:463-474; strings as at :420-421 / :431-432):
 *   contig_text/contig_len  the contig string (1 byte per character)
 *   chrom/chrom_len         the chromosome column text (CROPSR.py:422 chromosome[1::])
 *   pos[r], minus[r]        regex match index and strand (0 '+', 1 '-') of row r
 *   score[r]                on_site_score of row r (ignored when long_sequence != 30 chars)
 *   ids                     n_rows x 7 bytes, the crispr_id of each row
 * Output: the CSV bytes ("\r\n" line ends, minimal quoting, repr() floats, 11-field rows
 * with -1 where the reference writes them).  Returns CRP_ERR_CAPACITY with the needed size
 * in *out_len when out_cap is too small. */
int crp_format_rows(const uint8_t *contig_text, uint64_t contig_len, const uint8_t *chrom, uint64_t chrom_len,
                    int guide_len, const uint32_t *pos, const uint8_t *minus, const double *score,
                    const uint8_t *ids, uint64_t n_rows, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                    int n_threads);

/* The same rows appended to an open file descriptor instead of a buffer: the stand-in for
 * csv.writer(file).writerows(rows) at CROPSR.py:471-474 when the rows of a chunk are not
 * wanted in memory.  n_threads workers format blocks of 16384 rows and commit them with
 * write(2) in row order (a descriptor opened with O_APPEND, like Python's mode "a", appends).
 * *bytes_written (may be NULL) receives the number of bytes written; on CRP_ERR_IO the output
 * stops at a block boundary.  Flush any buffered writer on the same file before the call. */
int crp_write_rows(int fd, const uint8_t *contig_text, uint64_t contig_len, const uint8_t *chrom, uint64_t chrom_len,
                   int guide_len, const uint32_t *pos, const uint8_t *minus, const double *score,
                   const uint8_t *ids, uint64_t n_rows, uint64_t *bytes_written, int n_threads);

/* The reference's own crispr ids (CROPSR.py:316-318: np.random.choice(alphanum, [n_rows, 7]) on
 * numpy's global legacy generator), drawn natively: mt_key[624] / *mt_pos are the MT19937 state
 * from np.random.get_state(); on return they hold the state after the draws, for set_state().
 * Same values, same state afterwards as numpy; reverse != 0 stores the rows last-first. */
int crp_legacy_ids(uint32_t *mt_key, int32_t *mt_pos, uint8_t *ids, uint64_t n_rows, int reverse);

/* ---- input side: FASTA bytes -> contig strings (host code, no GPU needed) ----- */
/* The contig table import_fasta_file builds (CROPSR.py:54-74 with cropsr_functions.py:221-229
 * and :190-196) for a file in the "re-formatted" path whose records all have a header line and
 * whose headers and bodies are plain (printable ASCII without blank, quote, backslash):
 *   data/n        the file's bytes as text mode hands them over (newlines already '\n')
 *   out_text      receives the VALUE strings back to back: for record k
 *                 ' + body without newlines + ') + (',' or, for the last record, ']')
 *                 -- the exact character string CROPSR.py:412-434 scans for that contig
 *   records       4 x uint64 per record: header offset and length in `data`, value offset and
 *                 length in `out_text` (the host prepends  [('  or  ('  and appends  ',  to the
 *                 header to get the dict key, and applies dict semantics to repeated keys)
 * *plain = 1 when the table was produced.  *plain = 0 (with CRP_OK) means the input is outside
 * this fast path -- already two lines per record, a header with a blank or quote, a record
 * without a newline, no record at all -- and the caller must build the table the literal way.
 * CRP_ERR_CAPACITY reports the needed sizes in *n_records / *out_len (out_cap >= n + 4 * records
 * always suffices).  Work is spread over n_threads threads in 4 MiB pieces of the input. */
int crp_fasta_table(const uint8_t *data, uint64_t n, uint8_t *out_text, uint64_t out_cap, uint64_t *records,
                    uint64_t records_cap, uint64_t *n_records, uint64_t *out_len, int *plain, int n_threads);

/* The same rows with the two OPT-IN extensions of this engine (both absent from the reference, whose
 * default output stays byte-identical when they are not asked for):
 *   features    the `features` column (always '' in the reference, CROPSR.py:466-468): a table of
 *               strings, entry t = feat_blob[feat_off[t] : feat_off[t+1]], and per row the entry it
 *               gets, feat_idx[r] (0xFFFFFFFF: ''); csv-quoted as needed.  feat_idx NULL = ''.
 *               Rows without a cutsite (the 11-field rows) keep ''.
 *   offtarget   4 x uint32 per row appended as four more columns (crp_offtarget_counts);
 *               0xFFFFFFFF prints as -1.  NULL = no extra columns.
 * With both NULL this is crp_write_rows. */
int crp_write_rows_ex(int fd, const uint8_t *contig_text, uint64_t contig_len, const uint8_t *chrom, uint64_t chrom_len,
                      int guide_len, const uint32_t *pos, const uint8_t *minus, const double *score,
                      const uint8_t *ids, uint64_t n_rows, const uint8_t *feat_blob, const uint64_t *feat_off,
                      const uint32_t *feat_idx, const uint32_t *offtarget, uint64_t *bytes_written, int n_threads);

/* Rows of several SEGMENTS -- a segment is what crp_write_rows_ex takes: consecutive rows of one contig with their columns --
 * appended to fd in segment order by ONE call: the rows a write pass of the reference sends through csv.writer.writerows
 * (CROPSR.py:442-474; with the reference's accumulating Complete_dataset, :407, a pass holds the rows of every contig so far),
 * or the passes of several short contigs together.  A worker's block (16384 rows, one write(2)) may span segments, so a run of
 * short contigs costs what one contig of their total size costs.  Bytes: exactly the concatenation of the segments'
 * crp_write_rows_ex output.  feat_idx / offtarget may be NULL per segment like there; guide_len is the call's. */
typedef struct crp_row_segment {
    const uint8_t *contig_text;
    uint64_t contig_len;
    const uint8_t *chrom;
    uint64_t chrom_len;
    const uint32_t *pos;
    const uint8_t *minus;
    const double *score;
    const uint8_t *ids;
    uint64_t n_rows;
    const uint8_t *feat_blob;
    const uint64_t *feat_off;
    const uint32_t *feat_idx;
    const uint32_t *offtarget;
} crp_row_segment;
int crp_write_segments(int fd, int guide_len, const crp_row_segment *segs, uint64_t n_segs, uint64_t *bytes_written, int n_threads);

/* The same with the OPT-IN genome-wide specificity columns of the CSV join (crp_search_self_join_hits; DESIGN.md section
 * 15, CSV join): extras, when not NULL, is an array parallel to segs.  An entry with self_counts == NULL adds nothing;
 * with extras == NULL the call is crp_write_segments.  Otherwise every row of the segment -- the 11-field rows too --
 * gets n_counts + 2 more fields, after the off-target fields if present: its n_counts counts (self_counts, n_counts per
 * row; 0xFFFFFFFF prints as -1), hit_sum (self_hit_sum, one per row, a decimal integer) and the specificity
 * 1 / (1 + hit_sum / 2^30) as repr(float); a hit_sum of 2^64 - 1, or self_hit_sum == NULL, prints -1 in both. */
typedef struct crp_row_extra {
    const uint32_t *self_counts;
    int n_counts;
    const uint64_t *self_hit_sum;
} crp_row_extra;
int crp_write_segments_cols(int fd, int guide_len, const crp_row_segment *segs, const crp_row_extra *extras, uint64_t n_segs,
                            uint64_t *bytes_written, int n_threads);

/* The same with the OPT-IN guide property columns (crp_guide_properties): props, when not NULL, is an
 * array parallel to segs of one pointer per segment -- the packed word of every row of the segment, or NULL, which adds
 * nothing; with props == NULL the call is crp_write_segments_cols.  Every row of such a segment -- the 11-field rows too
 * -- gets four more decimal integer fields, after the specificity fields if present: guide_gc, guide_run, guide_t_run,
 * guide_stem. */
int crp_write_segments_props(int fd, int guide_len, const crp_row_segment *segs, const crp_row_extra *extras,
                             const uint32_t *const *props, uint64_t n_segs, uint64_t *bytes_written, int n_threads);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------ */
/* The reference has no parallelism (its only hint is the dead cropsr_functions.py:256-273).  The path
 * shards by contig with no collective on the data path; the one exchange is the final gatherv of the
 * per-rank hit tables to a root.  RCCL has no gatherv: crp_gather_hits does an all-gather of the two
 * counts, then ncclGroupStart / ncclSend|ncclRecv per column / ncclGroupEnd -- every peer->root
 * transfer on its own xGMI link.  librccl.so is loaded on the first crp_comm_* call, never before.
 * The 128-byte id comes from crp_comm_unique_id on one rank and reaches the others through the
 * launcher (cropsr_amd/rendezvous.py: a socket of its own, not torch). */
#define CRP_COMM_ID_BYTES 128
int crp_comm_unique_id(uint8_t id[CRP_COMM_ID_BYTES]);
int crp_comm_init(crp_ctx *ctx, const uint8_t id[CRP_COMM_ID_BYTES], int rank, int world);
int crp_comm_destroy(crp_ctx *ctx);
/* All ranks: returns when every rank has called it and the library's stream has drained. */
int crp_comm_barrier(crp_ctx *ctx);
/* Element-wise reduction of n (<= 64) host doubles over all ranks, result on every rank. */
#define CRP_REDUCE_SUM 0
#define CRP_REDUCE_MAX 1
int crp_comm_allreduce_f64(crp_ctx *ctx, double *values, int n, int op);
/* All ranks, after crp_scan_score on `arena` (NULL: this rank contributes empty tables): gathers the
 * '+' and '-' tables (pos u32, score f64) of every rank into root's HBM.  flags (the same on every
 * rank): CRP_GATHER_OFFTARGET also gathers the per-hit off-target counts (crp_offtarget_counts must
 * have run on `arena`).  counts_all (2 x world values, may be NULL) receives every rank's
 * {n_plus, n_minus} on every rank.
 * Failure is collective: whatever can go wrong on ONE rank before the tables move -- its arena has no
 * (matching) tables: CRP_ERR_STATE; the root cannot size its receive buffers: CRP_ERR_NOMEM -- travels with
 * the counts, and every rank returns from the same call without starting the exchange: the rank at fault with
 * its own status, the others with CRP_ERR_PEER (crp_last_error names the rank).  The communicator stays
 * usable.  CRP_ERR_COMM / CRP_ERR_HIP from inside the exchange are NOT agreed on: the caller must end the run. */
#define CRP_GATHER_OFFTARGET 1
/* CRP_GATHER_PRE: the f64 column that travels is the pre-sigmoid sum (crp_scan_score with want_pre)
 * instead of the score -- for a root that applies its own host's exp (cli --score-finalize=host). */
#define CRP_GATHER_PRE 2
/* CRP_GATHER_FEATURES: also gathers the per-hit label-set ids of the annotation join (crp_annotate_lookup must
 * have run on `arena` since its last scan; else CRP_ERR_STATE, agreed on like the others). */
#define CRP_GATHER_FEATURES 4
/* CRP_GATHER_POS16: positions cross the links as 16 bits per hit plus one uint32 per 65 536 arena positions (the index of
 * the first hit at or after it) instead of 32 bits per hit -- tables are ascending, so this is exact and needs no escape:
 * 10 B per hit instead of 12.  A small kernel packs on the peers, another expands into the root's table
 * (crp_gather.hip); what crp_gathered_fetch returns is bit for bit the same. */
#define CRP_GATHER_POS16 8
int crp_gather_hits(crp_ctx *ctx, crp_arena *arena, int root, int flags, uint64_t *counts_all);
/* Root only: copy the tables rank `rank` contributed to the last crp_gather_hits to host arrays
 * (sizes from counts_all; ot_*: 4 x uint32 per hit; any pointer may be NULL). */
int crp_gathered_fetch(crp_ctx *ctx, int rank, uint32_t *pos_plus, double *score_plus, uint32_t *ot_plus,
                       uint32_t *pos_minus, double *score_minus, uint32_t *ot_minus);

/* Root only, after a crp_gather_hits with CRP_GATHER_FEATURES: the ids rank `rank` contributed (uint32 per hit). */
int crp_gathered_fetch_features(crp_ctx *ctx, int rank, uint32_t *feat_plus, uint32_t *feat_minus);

/* ---- seam 1 as a pipeline: upload | scan | fetch side by side ---------------- */
/* The reference's loop produces and consumes contig by contig (CROPSR.py:409-474).  crp_arena_* + crp_scan_score +
 * crp_fetch_hits do the three steps of seam 1 one after the other; crp_scan_stream does them as a pipeline over slices
 * of the genome (slice_chars characters each, 0 = 64 Mi; whole contigs while they fit, a longer contig cut with
 * CRP_HALO characters of context either side and every hit owned by the piece its match index falls in): while slice k is
 * scanned, slice k + 1 crosses the host link upwards and the tables of slice k - 1 cross it downwards.  One blocking
 * call; the caller's strings are read, not kept.
 *   texts / lens / n   the contig strings CROPSR.py:409 iterates over, in order (each at most 2^32 - 1 characters)
 *   flags              CRP_SCAN_PRE: the f64 column is the pre-sigmoid sum (CROPSR.py:312) instead of the score
 *   pos_* / score_*    the caller's tables, cap_* rows each (a pointer may be NULL: that column is not copied): ONE table
 *                      per strand, contig after contig, ascending inside a contig, positions LOCAL to the contig string
 *                      (the regex match indices of CROPSR.py:418 / :429) -- what crp_node_fetch returns.  Pinned memory
 *                      (crp_host_alloc) is written by DMA directly; pageable memory through the staging buffers.
 *   per_contig         2 x n values {plus, minus} (may be NULL); *n_plus / *n_minus: the totals
 *   stats              12 doubles (may be NULL): wall seconds, uploader busy, drainer busy (incl. waiting for the scans),
 *                      slices, lanes, seconds until the first slice's tables were on the host, uploader waiting for a
 *                      lane, drainer waiting for a staging buffer, copier busy (staging -> the caller's pageable tables),
 *                      copier waiting for the D2H copies, bytes the copier moved, 1 if the tables were pinned
 * CRP_ERR_CAPACITY: a table was too small -- nothing was written beyond cap_*, *n_plus / *n_minus hold the sizes to
 * come back with.  crp_scan_stream_prepare opens the pipeline's lanes (further contexts on the device -- four lanes in all,
 * environment CRP_STREAM_LANES 2..8 -- each with an arena of slice_chars and its tables) ahead of time, e.g. while the
 * FASTA is still being read. */
int crp_scan_stream(crp_ctx *ctx, const uint8_t *const *texts, const uint64_t *lens, uint64_t n, int guide_len, int flags,
                    uint64_t slice_chars, uint32_t *pos_plus, double *score_plus, uint64_t cap_plus, uint32_t *pos_minus,
                    double *score_minus, uint64_t cap_minus, uint64_t *per_contig, uint64_t *n_plus, uint64_t *n_minus,
                    double *stats);
int crp_scan_stream_prepare(crp_ctx *ctx, uint64_t slice_chars);
/* Host memory the GPU reaches by DMA (hipHostMalloc): tables allocated here are filled by crp_fetch_hits,
 * crp_node_fetch and crp_scan_stream without a staging copy and without first-touch page faults, and contig strings kept
 * here are uploaded straight off their pages (they must then stay valid until crp_arena_seal / the end of
 * crp_scan_stream).  For callers that keep their buffers from genome to genome: pinning costs more than one copy saves. */
int crp_host_alloc(uint64_t bytes, void **out);
int crp_host_free(void *p);

/* ---- multi-GPU: ONE process over N GPUs, the node handle -------------------- */
/* The reference is one process with one contig loop (CROPSR.py:333, :409).  A crp_node lets that one process drive N
 * GPUs through one handle: crp_node_load cuts the genome into N contiguous equal shares (a contig that straddles a
 * share boundary is cut there; every piece carries CRP_HALO characters of context either side, a hit belongs to the
 * piece that contains its match index) and uploads every share to its device; crp_node_scan_score launches the scan on
 * every device from a host thread of that device's own, so the kernels start side by side; crp_node_gather is the path's one exchange, the gatherv of the per-device tables
 * to a root device -- RCCL in one process (ncclCommInitAll; per peer ncclSend, at the root ncclRecv, all inside one
 * ncclGroupStart / ncclGroupEnd) or, where RCCL cannot run (the same device listed twice: rehearsals on one GPU) or is
 * not wanted, device-to-device copies the root pulls over its own streams, one per peer.  The root ends up with ONE
 * table per strand, in contig order, positions LOCAL to their contig string: exactly the regex match indices the
 * reference iterates over, bit for bit what one GPU alone produces.  The per-device crp_ctx / crp_arena stay
 * reachable (crp_node_ctx / crp_node_arena) for crp_configure, crp_profile_*, crp_device_info and the like. */
#define CRP_HALO 128
typedef struct crp_node crp_node;
/* Host side (no GPU needed): the cut.  lens[0..n): contig string lengths, in order.  Device r gets the characters
 * [r, r + 1) * total / world of the concatenation; a contig that straddles a boundary is cut there unless one side
 * would be shorter than min_piece (0: 4096) -- then it stays whole on the side that holds most of it.  pieces: 4 x uint64
 * per piece {contig, start, end, device}, in contig order; CRP_ERR_CAPACITY with the needed count in *n_pieces when cap
 * (in pieces) is too small.  At most n + world - 1 pieces. */
int crp_plan_shares(const uint64_t *lens, uint64_t n, int world, uint64_t min_piece, uint64_t *pieces, uint64_t cap,
                    uint64_t *n_pieces);
/* Opens the listed HIP devices (indices as this process sees them; the same index may appear more than once: each
 * entry is a logical device with a context of its own). */
int crp_node_init(int n_devices, const int *device_ids, crp_node **out);
int crp_node_destroy(crp_node *node);
/* Text of the last failure on the node or on one of its devices. */
const char *crp_node_last_error(const crp_node *node);
int crp_node_size(const crp_node *node);           /* number of logical devices (negative status on a NULL handle) */
crp_ctx *crp_node_ctx(crp_node *node, int k);      /* logical device k's context (NULL: out of range) */
crp_arena *crp_node_arena(crp_node *node, int k);  /* its (first) arena after crp_node_load (NULL: none -- the device got no piece) */
/* A device's share is packed into as many arenas as it needs (one arena addresses fewer than 2^31 characters; the
 * reference reads a genome of any size whole, CROPSR.py:59): a share beyond one arena goes on in the next, and a piece that
 * no arena can hold is cut again, with halos like every other cut.  Scan, the two opt-in steps, the ownership cuts and the
 * gatherv run arena by arena inside the library; the caller sees one table per strand as before.  crp_node_arenas: how
 * many arenas logical device k holds (negative status: bad argument); crp_node_arena_at: its j-th one. */
int crp_node_arenas(const crp_node *node, int k);
crp_arena *crp_node_arena_at(crp_node *node, int k, int j);
/* Knobs of a node (the environment sets the defaults at crp_node_init):
 *   CRP_NODE_OPT_ARENA_WORDS            most 64-character words one arena of the node may hold; 0 = crp_arena_max_words().
 *                                       Smaller values only make more arenas (tests; a way to bound one allocation).
 *   CRP_NODE_OPT_COMM_INIT_TIMEOUT_MS   how long ncclCommInitAll may take (it runs on a helper thread; default 180 000,
 *                                       environment CRP_NODE_COMM_INIT_TIMEOUT_S): a bootstrap that has not returned by then
 *                                       is left behind (crp_node_comm_stuck) and the node goes on as device-to-device
 *                                       copies, or fails with CRP_ERR_COMM if RCCL was asked for by name
 *                                       (CRP_NODE_TRANSPORT=rccl).  <= 0: no bound.
 *   CRP_NODE_OPT_COLLECTIVE_TIMEOUT_MS  how long the grouped send/recv of crp_node_gather and the histogram all-reduce
 *                                       of crp_node_offtarget may take (default 300 000, environment
 *                                       CRP_NODE_COLLECTIVE_TIMEOUT_S): RCCL has no time-out of its own, so the streams are
 *                                       awaited by polling an event.  When the bound runs out the communicators are
 *                                       aborted (ncclCommAbort) and never used again by this node; the call then starts over
 *                                       on the device-to-device transport from fresh state and returns CRP_OK (crp_node_last_error
 *                                       and crp_node_transport_note say what happened) -- or, with CRP_NODE_TRANSPORT=rccl,
 *                                       returns CRP_ERR_COMM naming the stage.  <= 0: no bound. */
#define CRP_NODE_OPT_ARENA_WORDS 1
#define CRP_NODE_OPT_COMM_INIT_TIMEOUT_MS 2
#define CRP_NODE_OPT_COLLECTIVE_TIMEOUT_MS 3
int crp_node_set_option(crp_node *node, int option, int64_t value);
/* Why RCCL is not (or no longer) this node's transport -- "" while it is, or was never wanted. */
const char *crp_node_transport_note(const crp_node *node);
/* Communicator bootstraps of this PROCESS that never returned: their helper threads still sit inside RCCL, and the
 * runtime's tear-down at a normal exit may wait for them -- a program that sees a non-zero value should flush its output
 * and leave through _exit (cropsr_amd/cli.py does). */
int crp_node_comm_stuck(void);
/* The genome: n contig strings, in order (the strings CROPSR.py:409 iterates over).  Cuts (crp_plan_shares), uploads
 * share r to device r (one host thread per device), seals.  The caller's strings are read, not kept.  A second call
 * replaces the genome.  Any total size; a single contig string may have at most 2^32 - 1 characters (the tables carry
 * contig-local positions as 32 bits): CRP_ERR_CAPACITY names a longer one. */
int crp_node_load(crp_node *node, const uint8_t *const *texts, const uint64_t *lens, uint64_t n);
/* The cut that was made: 7 x uint64 per piece {contig, start, end, device, arena offset of the piece's text in its
 * arena, index of `start` inside that text (the left halo's length), which of the device's arenas}.  Same capacity
 * protocol as crp_plan_shares; at most n + world - 1 pieces plus one per arena beyond a device's first. */
int crp_node_plan(const crp_node *node, uint64_t *pieces, uint64_t cap, uint64_t *n_pieces);
/* crp_scan_score on every device at once (same guide_len / flags).  *n_plus / *n_minus (may be NULL): rows of all
 * devices' tables together, INCLUDING the few hits inside halos (at most 2 x CRP_HALO positions per device); the
 * exact totals come from crp_node_gather. */
int crp_node_scan_score(crp_node *node, int guide_len, int flags, uint64_t *n_plus, uint64_t *n_minus);
/* The two opt-in steps over the node's resident tables, between crp_node_scan_score and crp_node_gather:
 *   crp_node_offtarget   the genome-wide off-target seed scan (see crp_offtarget_* below): every device adds the sites it
 *                        OWNS to its histogram (scan with CRP_SCAN_SEEDS to hand the seed words over), the histograms
 *                        are summed over the devices (RCCL all-reduce in one group; through device 0 when RCCL cannot
 *                        run), every device solves and looks up its own hits.  *n_sites (may be NULL): sites in all.
 *   crp_node_annotate    the annotation join (see crp_annotate_* below) on every device with the track of ITS pieces:
 *                        seqid_of_contig[k] = index of contig k's FASTA name among the annotation's seqids
 *                        (crp_annotation_seqid order; any value >= their number: no features), dec as in
 *                        crp_annotation_track.
 * The counts / ids stay in HBM and travel with crp_node_gather (CRP_GATHER_OFFTARGET / CRP_GATHER_FEATURES). */
struct crp_annotation;
int crp_node_offtarget(crp_node *node, int guide_len, uint64_t *n_sites);
int crp_node_annotate(crp_node *node, const struct crp_annotation *annotation, const uint64_t *seqid_of_contig, int dec);
/* The gatherv: every device's OWNED rows to logical device `root`.  flags: CRP_GATHER_PRE (the f64 column is the
 * pre-sigmoid sum), CRP_GATHER_POS16 (10 B per hit on the links instead of 12, see above), CRP_GATHER_OFFTARGET /
 * CRP_GATHER_FEATURES (the columns of the two steps above travel too),
 * CRP_NODE_PEER_COPY (device-to-device copies instead of RCCL for this call; always the case when a device is
 * listed twice, or when the environment says CRP_NODE_TRANSPORT=peer).  CRP_NODE_TRANSPORT=rccl: RCCL or CRP_ERR_COMM (no
 * falling back; also with a device listed twice, where the real RCCL refuses the clique); CRP_NODE_TRANSPORT=try: RCCL
 * is attempted even with a device listed twice and given up for device-to-device copies like in the default mode. */
#define CRP_NODE_PEER_COPY 16
/* CRP_NODE_HOST_GATHER: for a consumer that lives on the HOST (the reference's consumer does: csv.writer, CROPSR.py:471-474).
 * Nothing crosses xGMI and no table is built on `root`: the call makes the ownership cuts and the counts, every device
 * rebases the positions of its owned rows where they lie, and crp_node_fetch (/_fetch_offtarget /_fetch_features) then
 * copies every device's rows over THAT device's own PCIe link, side by side, straight into their place in the caller's
 * arrays -- N host links instead of a gather into one GPU followed by one link.  Same rows, same order.
 * crp_node_tables_device has nothing to hand out after such a gather (CRP_ERR_STATE). */
#define CRP_NODE_HOST_GATHER 32
int crp_node_gather(crp_node *node, int root, int flags);
/* After crp_node_gather: kept hits per contig and strand (2 x n contigs: {plus, minus}) and in all; any pointer may
 * be NULL. */
int crp_node_counts(const crp_node *node, uint64_t *per_contig, uint64_t *n_plus, uint64_t *n_minus);
/* Rows of the gathered tables that carry a real score (not -1), counted on the root: the unit of "gRNAs scored". */
int crp_node_count_scored(crp_node *node, uint64_t *n_scored);
/* The gathered tables to host arrays (n_plus / n_minus rows; contig order, ascending inside a contig, positions local
 * to the contig string; any pointer may be NULL), and their addresses in the root's HBM (valid until the next
 * crp_node_gather / crp_node_load). */
int crp_node_fetch(crp_node *node, uint32_t *pos_plus, double *score_plus, uint32_t *pos_minus, double *score_minus);
int crp_node_tables_device(crp_node *node, void **pos_plus, void **score_plus, void **pos_minus, void **score_minus);
/* After a gather with CRP_GATHER_OFFTARGET / CRP_GATHER_FEATURES: the off-target counts (4 x uint32 per row) and the
 * label-set ids (uint32 per row) of the same rows, same order.  Either pointer may be NULL. */
int crp_node_fetch_offtarget(crp_node *node, uint32_t *ot_plus, uint32_t *ot_minus);
int crp_node_fetch_features(crp_node *node, uint32_t *feat_plus, uint32_t *feat_minus);
/* The last crp_node_gather in numbers: wall time of the whole call and of its exchange step alone (ms), bytes that
 * crossed from peers to the root, transport used (1 RCCL, 2 device-to-device copies, 3 none: host gather).  Any pointer may be NULL. */
#define CRP_TRANSPORT_RCCL 1
#define CRP_TRANSPORT_PEER_COPY 2
#define CRP_TRANSPORT_HOST_LINKS 3   /* CRP_NODE_HOST_GATHER: nothing moved between devices */
int crp_node_gather_stats(const crp_node *node, double *ms_total, double *ms_exchange, uint64_t *bytes_to_root, int *transport);

/* ---- annotation join (opt-in; a no-op in the reference) -------------------- */
/* BASELINE.json configs[2], [3] name a GFF and a Phytozome annotation_info file.  The reference parses the GFF
 * (CROPSR.py:77-95, called at :375), drops the table and writes '' into `features` (:466, :468), so the join is
 * this engine's own, opt-in, and the default CSV stays byte-identical (definition: cropsr_amd/annotate.py,
 * DESIGN.md section 11; parity unpinned).  The host builds, per arena, a TRACK: strictly ascending arena positions
 * points[k], each opening an elementary interval [points[k], points[k+1]) whose set of gene / CDS labels is
 * constant and named by ids[k] (an index into the caller's string table, or CRP_NO_FEATURE for "none"; every
 * contig starts with a point of its own, so nothing leaks from its predecessor).  The library keeps a copy in HBM
 * together with a bucket index over the arena's positions. */
#define CRP_NO_FEATURE 0xFFFFFFFFu
/* Host side (no GPU needed).  GFF3 bytes (+ the bytes of a Phytozome annotation_info file, or NULL) as text mode hands
 * them over -> the annotation: the distinct label-set strings and, per seqid, the elementary intervals of its gene /
 * CDS rows.  The definition (which rows, which label, which order) is stated at the top of
 * cropsr_amd/csrc/crp_annotation.cpp and restated as a brute-force loop in oracle/annotate_oracle.py. */
typedef struct crp_annotation crp_annotation;
int crp_annotation_build(const uint8_t *gff, uint64_t gff_len, const uint8_t *info_text, uint64_t info_len,
                         crp_annotation **out);
int crp_annotation_destroy(crp_annotation *annotation);
/* Sizes: seqids with at least one gene / CDS row, distinct label-set strings, bytes of all strings, gene and CDS
 * rows read (any pointer may be NULL). */
int crp_annotation_stats(const crp_annotation *annotation, uint64_t *n_seqids, uint64_t *n_strings, uint64_t *blob_bytes,
                         uint64_t *n_genes, uint64_t *n_cds);
/* The string table in the form crp_write_rows_ex takes: blob (blob_bytes) and n_strings + 1 offsets. */
int crp_annotation_strings(const crp_annotation *annotation, uint8_t *blob, uint64_t *offsets);
/* Seqid k (order of first appearance in the GFF): its name and its intervals in 1-based genome coordinates --
 * interval j = [points[j], points[j+1]) carries string ids[j] (CRP_NO_FEATURE: none).  The pointers stay valid
 * until crp_annotation_destroy. */
int crp_annotation_seqid(const crp_annotation *annotation, uint64_t k, const uint8_t **name, uint64_t *name_len,
                         const int64_t **points, const uint32_t **ids, uint64_t *n_points);
/* The track of one arena for crp_annotate_set_track.  entries: 4 x uint64 per text of the arena, in arena order --
 * {seqid index (any value >= n_seqids: the text has no features), index of the text's first character inside its
 * contig string (0 unless the text is a piece of a cut contig), length of the text, arena offset of the text}.
 * dec: the contig strings start with `dec` decoration characters before the first base (1 in the reference's
 * re-formatted path, 0 otherwise): string index = 1-based genome coordinate + dec - 1.
 * Every text opens with a point of its own.  Returns CRP_ERR_CAPACITY with the needed size in *n_out when cap is
 * too small (cap 0: sizing call). */
int crp_annotation_track(const crp_annotation *annotation, const uint64_t *entries, uint64_t n_entries, int dec,
                         uint32_t *points, uint32_t *ids, uint64_t cap, uint64_t *n_out);
/* Device side. */
int crp_annotate_set_track(crp_arena *arena, const uint32_t *points, const uint32_t *ids, uint64_t n_points);
/* After crp_scan_score on `arena` (whose tables it reads where they lie): per kept hit the id of the interval its
 * cut site falls in -- cut site = end_pos - 3 (CROPSR.py:155-158): i - 3 on the '+' table, j on the '-' table --
 * or CRP_NO_FEATURE for a hit before the first point and for a row WITHOUT a cut site (long_sequence is not 30
 * characters, CROPSR.py:466-468: exactly the rows whose score is -1).  One streaming pass over the position and
 * score columns (12 B in, 4 B out per hit).  The ids stay in HBM for crp_gather_hits(CRP_GATHER_FEATURES) and
 * are copied to feat_plus / feat_minus (n_plus / n_minus values, table order; either may be NULL); they are what
 * crp_write_rows_ex takes as feat_idx. */
int crp_annotate_lookup(crp_arena *arena, uint32_t *feat_plus, uint32_t *feat_minus);

/* ---- off-target seed scan (opt-in; absent from the reference) ------------- */
/* BASELINE.json configs[4]: genome-wide off-target <=3-mismatch seed scan.  The reference has no such
 * step (its only alignment code is the dead bowtie2 shell-out of prmrdsgn2.py:139-160), so the
 * definition is this engine's own, stated on the reference's own strings:
 *   site   every kept hit of the scan (either strand, CROPSR.py:419/:430) whose `sequence` column
 *          (CROPSR.py:420/:431) has >= 12 characters of which the first 12 -- the PAM-proximal seed --
 *          are bases after the scoring transform of CROPSR.py:458 (.replace('U','T').upper() in ACGT)
 *   count  for a site g and k = 0..3: the number of OTHER sites whose seed differs from g's in
 *          exactly k of the 12 positions
 * Genome-wide means: over every arena added between crp_offtarget_reset and crp_offtarget_solve, on
 * every rank of the communicator (crp_offtarget_reduce).  Method: a histogram of the 4^12 seeds (built
 * by partitioning the sites by seed prefix, no atomic per site), then
 * the exact Hamming-ball sums of that histogram for all seeds at once by a position-wise recurrence
 * (three passes of four positions through LDS), then one 16-byte look-up per hit -- no pairwise
 * comparison anywhere. */
#define CRP_OT_SEED_LEN 12
#define CRP_OT_MAX_MM 3
/* Allocates (first call) and zeroes the site histogram of this context. */
int crp_offtarget_reset(crp_ctx *ctx);
/* After crp_scan_score on `arena`: derives the seed of every kept hit and adds the sites to the
 * histogram.  own_ranges (n_ranges pairs [begin, end) of arena positions, ascending, may be NULL =
 * everything): only hits whose match position lies inside count as sites -- a contig cut into pieces
 * with halos (multi-GPU) must not count its halo hits twice.  *n_sites (may be NULL): sites added. */
int crp_offtarget_add(crp_arena *arena, int guide_len, const uint64_t *own_ranges, uint64_t n_ranges,
                      uint64_t *n_sites);
/* Multi-GPU: RCCL all-reduce (sum) of the histogram over the communicator -- the one bandwidth-heavy
 * xGMI collective of this engine (64 MiB per rank).  Without a communicator: no-op. */
int crp_offtarget_reduce(crp_ctx *ctx);
/* The site histogram (4^12 uint32) to / from host memory: what a host-side exchange sums instead of
 * crp_offtarget_reduce (ranks sharing one GPU, where RCCL cannot run), and what the tests check. */
int crp_offtarget_hist_get(crp_ctx *ctx, uint32_t *hist);
int crp_offtarget_hist_set(crp_ctx *ctx, const uint32_t *hist);
/* Hamming-ball sums for all 4^12 seeds. */
int crp_offtarget_solve(crp_ctx *ctx);
/* Per-hit counts of `arena` (which must have been added): 4 x uint32 per hit, table order, k = 0..3;
 * 0xFFFFFFFF x 4 for a hit that is not a site.  Host pointers may be NULL (counts stay in HBM). */
int crp_offtarget_counts(crp_arena *arena, uint32_t *counts_plus, uint32_t *counts_minus);
/* The seed codes of the same hits (uint32 per hit: sum of code_k << 2k, A=0 T=1 C=2 G=3, k = 0 next
 * to the PAM; 0xFFFFFFFF not a site, 0xFFFFFFFE a site outside own_ranges), for tests. */
int crp_offtarget_seeds(crp_arena *arena, uint32_t *seeds_plus, uint32_t *seeds_minus);

/* ---- off-target search of given guides --------------- */
/* Every site of an arena that fits a PAM pattern, on both strands, within max_mm mismatches of each
 * query guide (a Cas-OFFinder-style search; not reference behaviour).
 *   pattern  T letters (1 <= T <= CRP_SEARCH_MAX_T) of ACGTRYSWKMBDHVN, either case, 5' -> 3' on the
 *            target strand.
 *   site     the window of T characters at forward arena start i (strand '+'), or its reverse complement
 *            (strand '-'), inside one contig (no void character); every pattern position whose letter is
 *            not N holds a base (acgtACGT, U read as A) of that letter's set.
 *   query    T letters of ACGTN, either case; the mismatches at a site are the positions where the query
 *            has a base and the oriented site does not hold that base (a non-base character always
 *            mismatches); query N positions are not compared.
 * A handle works on one sealed arena, which must outlive it.  Candidates (16 B each) are kept in HBM
 * within a budget (crp_search_set_budget, default CRP_SEARCH_DEFAULT_BUDGET bytes): an arena with more
 * candidates is processed in chunks, each run extracting them again.  Queries are compared in batches
 * sized so that one launch stays in the tens of milliseconds (at most 2^36 pairs and 4096 queries).  Invalid input: CRP_ERR_INVALID (NULL,
 * a letter outside the alphabet) or CRP_ERR_UNSUPPORTED (T outside 1..32, max_mm outside 0..8,
 * 2^28 or more queries). */
typedef struct crp_search crp_search;
#define CRP_SEARCH_MAX_T 32
#define CRP_SEARCH_MAX_MM 8
#define CRP_SEARCH_DEFAULT_BUDGET (4ull << 30)
/* Validates the pattern and counts the arena's candidates on the device (CRP_ERR_STATE: not sealed). */
int crp_search_create(crp_arena *arena, const char *pattern, int pattern_len, crp_search **out);
int crp_search_destroy(crp_search *search);
/* Device bytes the candidates of one chunk may take (0 = the default; at least one workgroup's worth,
 * 512 KiB, is always allowed).  Takes effect at the next run. */
int crp_search_set_budget(crp_search *search, uint64_t bytes);
/* At most batch_queries queries per compare launch (0 = the default, 4096; fewer launches than that
 * also keep each launch within 2^36 pairs), and first_site_slots sites in the device list a run starts
 * with (0 = the default, 2^20; a run that finds more repeats its compare once with room for all of
 * them).  Results do not depend on either; they bound launch length and memory. */
int crp_search_set_limits(crp_search *search, uint64_t batch_queries, uint64_t first_site_slots);
/* Candidate sites of the arena on each strand. */
int crp_search_candidates(const crp_search *search, uint64_t *n_plus, uint64_t *n_minus);
/* Runs n_queries queries (n_queries * T characters, query after query).  counts (n_queries * (max_mm + 1)
 * uint32, may be NULL) receives the sites per query with exactly k mismatches at [q * (max_mm + 1) + k];
 * *n_sites the number of sites.  When that exceeds site_cap the counts are still exact, nothing can be
 * fetched and the call returns CRP_ERR_CAPACITY: a run with site_cap >= *n_sites returns the full list. */
int crp_search_run(crp_search *search, const char *queries, uint64_t n_queries, int max_mm, uint64_t site_cap,
                   uint32_t *counts, uint64_t *n_sites);
/* The sites of the last successful run, ordered by query, arena position, strand ('+' first): query
 * index, forward arena start, strand (0 '+', 1 '-'), mismatches.  Any pointer may be NULL.
 * CRP_ERR_CAPACITY when cap < the number of sites; CRP_ERR_STATE without such a run. */
int crp_search_fetch(const crp_search *search, uint32_t *query, uint32_t *arena_pos, uint8_t *strand, uint8_t *mismatches,
                     uint64_t cap);
/* Bulges (Bulges).  A DNA bulge of d is d genomic bases that stay unpaired, an RNA
 * bulge of r is r query letters with no genomic partner.  The handle's pattern is the window pattern of one
 * bulge kind: T + d letters (DNA) or T - r (RNA) for queries of T letters, i.e. the query's pattern with d more
 * (r fewer) N in its guide region.  span: 2 bytes per query, the query positions of the first and last base of
 * its span (the guide region's first to last ACGT letter).  A placement s is the query position where the
 * bulge starts: span_first < s <= span_last (DNA), span_first < s and s + r - 1 < span_last (RNA).  Query
 * position i pairs with window position i when i < s, else with i + d (DNA) or i - r (RNA; positions s ..
 * s + r - 1 pair with nothing); mismatches count over the paired positions as in crp_search_run.  Each site
 * keeps its fewest mismatches over s, reported when <= max_mm, with bulge_at = s - span_first for the smallest
 * s that reaches them. */
#define CRP_SEARCH_BULGE_DNA 1
#define CRP_SEARCH_BULGE_RNA 2
#define CRP_SEARCH_MAX_BULGE 2
/* crp_search_run for one bulge kind (kind CRP_SEARCH_BULGE_DNA / _RNA, size 1..CRP_SEARCH_MAX_BULGE):
 * n_queries queries of T letters (T = the pattern's length - size for DNA, + size for RNA, at most 32), counts
 * and the capacity protocol as there.  One site per (query, position, strand).  Fewer than 2^23 queries (the
 * site word also carries the placement).  CRP_ERR_INVALID: a span without a placement or past the query;
 * CRP_ERR_UNSUPPORTED: kind size, max_mm, T or n_queries out of range.  Launches cover at most 2^35 pairs. */
int crp_search_run_bulge(crp_search *search, const char *queries, uint64_t n_queries, int kind, int size, const uint8_t *span,
                         int max_mm, uint64_t site_cap, uint32_t *counts, uint64_t *n_sites);
/* crp_search_fetch plus bulge_at (0 after a crp_search_run); order: query, arena position, strand. */
int crp_search_fetch_bulge(const crp_search *search, uint32_t *query, uint32_t *arena_pos, uint8_t *strand, uint8_t *mismatches,
                           uint8_t *bulge_at, uint64_t cap);
/* Specificity score (Specificity score).  A scheme weighs every hit of a query by where its
 * mismatches sit.  The guide region is the n_factor pattern positions outside the PAM, which is the pattern's last
 * T - n_factor positions (CRP_SEARCH_PAM_3PRIME) or its first (CRP_SEARCH_PAM_5PRIME); its positions are numbered
 * g = 0 .. n_factor - 1 from the PAM-distal end, so g = n_factor - 1 is next to the PAM on either side.  For a hit
 * with n >= 1 mismatches at g1 < g2 < .. < gn,
 *   h = factor[g1] * factor[g2] * .. * factor[gn] * shape[n * 32 + (gn - g1)]   (float64, left to right)
 *   v = (uint64) rint(h * 2^30)                                                 (round to nearest even)
 * and hit_sum[q] is the sum of v over the query's sites with 1 .. max_mm mismatches: exact integers, independent of
 * the order the device finds them in.  Specificity = 1 / (1 + hit_sum / 2^30) is the caller's to form. */
#define CRP_SEARCH_PAM_3PRIME 0
#define CRP_SEARCH_PAM_5PRIME 1
#define CRP_SEARCH_SHAPE_DOUBLES 288 /* shape[n][d]: n = 0..8 mismatches, d = 0..31 = last - first mismatching g */
#define CRP_SEARCH_SCORE_ONE (1ull << 30)
/* Sets the handle's scheme: factor[n_factor] (1 <= n_factor <= T) and shape[CRP_SEARCH_SHAPE_DOUBLES], every value
 * finite and in [0, 1].  A NULL factor clears the scheme.  CRP_ERR_INVALID: a NULL shape, n_factor or pam_side out
 * of range, a value outside [0, 1] or not finite. */
int crp_search_set_scheme(crp_search *search, const double *factor, int n_factor, int pam_side, const double *shape);
/* crp_search_run plus hit_sum (n_queries uint64).  The capacity protocol is crp_search_run's, and like the counts
 * the sums are exact under CRP_ERR_CAPACITY: site_cap = 0 is the score-only run, which keeps no site list at all.
 * CRP_ERR_STATE without a scheme; CRP_ERR_INVALID for a query with a base outside the guide region (its
 * mismatches there would have no g). */
int crp_search_run_scored(crp_search *search, const char *queries, uint64_t n_queries, int max_mm, uint64_t site_cap,
                          uint32_t *counts, uint64_t *n_sites, uint64_t *hit_sum);
/* Pair table (Pair tables): the other form of a scheme, in which a mismatch costs by which query
 * letter faces which site letter, and the site's PAM letters weigh the whole hit (the CFD form).  pair[n_factor][4][4]
 * is indexed by g (as above), the query's letter and the oriented site's letter, both over A, C, G, T in that order; the
 * diagonal is ignored.  pam_offsets[n_pam_offsets] (0 .. CRP_SEARCH_PAIR_MAX_PAM of them, strictly ascending) are offsets
 * inside the PAM, 0 its 5'-most letter, each on a pattern letter other than N; pam[4^n_pam_offsets] is indexed by the
 * site's letters there, first offset most significant (no offsets: the PAM factor is 1, pam may be NULL).  For a hit
 * with n >= 1 mismatches at g1 < .. < gn,
 *   h = 1; h = h * pair[g][query letter][site letter] for g = g1 .. gn; h = h * pam[..]   (float64, one multiply a step)
 *   v = (uint64) rint(h * 2^30), and v = 0 when a mismatching position of the site holds no base.
 * Setting a pair table clears the handle's scheme and the other way round; crp_search_run_scored serves whichever is
 * set.  A NULL pair clears both.  CRP_ERR_INVALID: pam_side out of range, a guide region of n_factor positions on that
 * side that is not all N in the handle's pattern, a value outside [0, 1] or not finite, offsets outside the rule. */
#define CRP_SEARCH_PAIR_MAX_PAM 3
int crp_search_set_pair_scheme(crp_search *search, const double *pair, int n_factor, int pam_side, const int *pam_offsets,
                               int n_pam_offsets, const double *pam);
/* Measurement, accumulated since create: out[0] ms of candidate extraction (count and emit kernels),
 * out[1] ms of compare kernels, out[2] extraction launches, out[3] compare launches, out[4] chunks of the
 * current plan, out[5] device bytes of the candidate buffers.  n: how many of these to write (<= 6). */
int crp_search_stats(const crp_search *search, double *out, int n);

/* ---- self search: every guide site of the genome against every candidate site (Self search) -- */
/* A guide site is a site of guide_pattern (NULL: the pattern itself) whose guide region -- the pattern_len - pam_len
 * positions outside the PAM, all N in both patterns, the PAM being the last pam_len letters or, failing that, the
 * first -- holds bases only; every PAM letter of guide_pattern accepts a subset of what the pattern's accepts.  Its
 * row counts, for k = 0 .. max_mm, the candidate sites other than itself with exactly k mismatches over the guide
 * region, and with a scheme sums their values as crp_search_run_scored does.  The pairs are found through
 * max_mm + 1 orderings of the candidates, one per segment of the guide region (two windows within max_mm mismatches
 * agree in one of them), never by visiting all pairs.  A handle holds all candidates of its arena, one ordering and
 * one row per candidate in HBM: 45 + 4 (max_mm + 1) bytes per candidate. */
typedef struct crp_search_self crp_search_self;
#define CRP_SEARCH_SELF_MAX_MM 4
#define CRP_SEARCH_SELF_DEFAULT_BUDGET (64ull << 30)
/* Extracts the candidates and flags the guide sites.  budget: device bytes the handle may take (0 = the default);
 * *needed_bytes (may be NULL) receives what it takes, also when that exceeds the budget: CRP_ERR_CAPACITY, no
 * handle.  CRP_ERR_INVALID: a letter outside the alphabet, a guide region that is not all N, a guide pattern wider
 * than the pattern; CRP_ERR_UNSUPPORTED: max_mm outside 0..4, pattern_len outside 2..32, a guide region shorter than
 * max_mm + 1; CRP_ERR_STATE: arena not sealed. */
int crp_search_self_create(crp_arena *arena, const char *pattern, const char *guide_pattern, int pattern_len, int pam_len,
                           int max_mm, uint64_t budget, uint64_t *needed_bytes, crp_search_self **out);
int crp_search_self_destroy(crp_search_self *self);
/* At most pairs_per_launch pairs per compare launch (0 = the default and the most, 2^36; a launch holds at least one
 * work item of up to 256 guide sites x one slice of a bucket).  Results do not depend on it. */
int crp_search_self_set_limits(crp_search_self *self, uint64_t pairs_per_launch);
/* crp_search_set_scheme for the handle's rows: n_factor must be the guide region's length; the PAM's side is the
 * handle's.  A NULL factor clears the scheme. */
int crp_search_self_set_scheme(crp_search_self *self, const double *factor, int n_factor, const double *shape);
/* crp_search_set_pair_scheme for the handle's rows (n_factor: the guide region's length; the PAM's side is the
 * handle's).  The candidates' PAM letters are read from the candidates' handle at compare time. */
int crp_search_self_set_pair_scheme(crp_search_self *self, const double *pair, int n_factor, const int *pam_offsets,
                                    int n_pam_offsets, const double *pam);
int crp_search_self_sizes(const crp_search_self *self, uint64_t *n_plus, uint64_t *n_minus, uint64_t *n_guides);
/* Orders the handle's candidates by segment 0 .. max_mm of the guide region (replaces the ordering it held). */
int crp_search_self_order(crp_search_self *self, int segment);
/* The guide sites of `guides` against the candidates of `candidates` (the same handle, or another arena's with the
 * same patterns and max_mm), both ordered by the same segment (else CRP_ERR_STATE): every pair within max_mm
 * mismatches that agrees in this segment and in no earlier one adds to the row of its guide site.  A full search is,
 * for every segment, the orderings of all handles and then every ordered pair of handles. */
int crp_search_self_compare(crp_search_self *guides, crp_search_self *candidates);
/* The guide sites in extraction order (ascending 64-position word; within a word '+' sites ascending, then '-'):
 * forward arena start, strand (0 '+', 1 '-'), the oriented window's base codes (bit p of hi, lo = the high and low
 * code bit of pattern position p; A=00 T=01 C=10 G=11), counts (max_mm + 1 per site) and hit_sum.  Any pointer may
 * be NULL.  CRP_ERR_CAPACITY when cap < the number of guide sites. */
int crp_search_self_fetch(crp_search_self *self, uint32_t *arena_pos, uint8_t *strand, uint32_t *hi, uint32_t *lo,
                          uint32_t *counts, uint64_t *hit_sum, uint64_t cap);
/* Measurement, accumulated since create (compare figures on the `guides` handle): out[0] ms of extraction (count,
 * emit, guide flags), out[1] ms of ordering kernels, out[2] ms of compare kernels, out[3] compare launches, out[4]
 * the longest compare launch in ms, out[5] pairs compared, out[6] device bytes of the handle, out[7] ordering
 * launches, out[8] ms of the join kernels (crp_search_self_join_hits).  n: how many of these to write (<= 9). */
int crp_search_self_stats(const crp_search_self *self, double *out, int n);
/* ---- on-target model of every guide site (opt-in) ---- */
/* A position-specific linear model over the oriented site and the letters around it, for the handle's pattern of T letters
 * with a guide region of G = T - P:
 *   window   W letters (1 .. 64), `left` of them before pattern position 0 of the oriented site (0 <= left < W): window
 *            position w is pattern position w - left.  A '+' site with forward start s reads forward positions s - left ..
 *            s - left + W - 1; a '-' site reads s + T - 1 + left down to s + T + left - W, each complemented
 *   tables   single[w * 4 + b] (W x 4), pair[w * 16 + b1 * 4 + b2] ((W - 1) x 16, window letters w and w + 1) and gc[0 .. G]
 *            (n_gc = G + 1 weights, one per GC count of the guide region); letters in the order A T C G.  A NULL table is
 *            all 0.0
 *   sum      ((intercept + gc[GC]) + single[0] + .. + single[W - 1]) + pair[0] + .. + pair[W - 2] in f64, one add per term in
 *            that order, no fused multiply-add, no reassociation: a host loop in the same order gives the same bits
 *   no sum   a window position that is no base (its `ac` bit is clear: N, IUPAC letters, decoration, void, positions outside
 *            the planes) leaves the site without a sum: a quiet NaN (0x7FF8000000000000)
 * A link (logistic) is the caller's: the device never calls exp.
 * set_model: CRP_ERR_INVALID with a crp_last_error text and no side effect for W outside 1 .. 64, left outside 0 .. W - 1,
 * a gc table whose length is not G + 1, a weight that is not finite; CRP_ERR_CAPACITY when the sums' column (8 bytes a
 * candidate) does not fit the handle's budget.  A new model replaces the old one and its sums. */
int crp_search_self_set_model(crp_search_self *self, int window, int left, double intercept, const double *single, const double *pair,
                              const double *gc, int n_gc);
/* One f64 per candidate, on the device (one kernel).  Valid once the handle exists: it needs no order and no compare.
 * CRP_ERR_STATE without a model. */
int crp_search_self_run_model(crp_search_self *self);
/* The sums of the guide sites, in crp_search_self_fetch's order.  CRP_ERR_STATE before crp_search_self_run_model,
 * CRP_ERR_CAPACITY when cap < the number of guide sites. */
int crp_search_self_fetch_model(crp_search_self *self, double *sum, uint64_t cap);
/* Measurement of the last crp_search_self_run_model: out[0] ms of the kernel (HIP events), out[1] rows (candidates).  n: how
 * many to write (<= 2). */
int crp_search_self_model_stats(const crp_search_self *self, double *out, int n);
/* The CSV join (CSV join): the rows of the handle's guide sites, handed to the hits of the arena's
 * last crp_scan_score at guide length guide_len, after the handle's orders and compares.  The handle's pattern must have
 * guide_len + 3 letters with a PAM of 3 on the 3' side, so its guide region is what the scan calls `sequence`:
 *   '+' hit, match index i  its site is forward start i - guide_len, strand '+'
 *   '-' hit, match index j  its site is forward start j, strand '-'
 * A hit whose site is a guide site of the handle gets that site's counts[0 .. max_mm] and hit_sum; every other hit (its
 * site only a candidate, a guide-region character that is no base, a '-' window the contig end cuts) gets 0xFFFFFFFF in
 * every count and 2^64 - 1 as hit_sum.  A handle without a scheme joins the counts; its hit_sum column is all-ones.
 * The columns are in hit-table order ((max_mm + 1) counts per hit), stay in HBM on the handle until the next join or
 * destroy, and are copied to the host pointers given (each may be NULL).  One kernel lane per hit: a binary search over
 * the candidates in extraction order, no atomics.  CRP_ERR_INVALID with a crp_last_error text: pattern_len is not
 * guide_len + 3, the PAM is on the 5' side or not 3 letters, the arena has no tables of that guide length. */
int crp_search_self_join_hits(crp_search_self *self, int guide_len, uint32_t *counts_plus, uint64_t *hit_sum_plus,
                              uint32_t *counts_minus, uint64_t *hit_sum_minus);
/* Device addresses of the joined columns of the last crp_search_self_join_hits (CRP_ERR_STATE without one); any pointer
 * may be NULL. */
int crp_search_self_join_device(crp_search_self *self, void **counts_plus, void **hit_sum_plus, void **counts_minus,
                                void **hit_sum_minus);

/* ---- gene families on a self-search handle ------------------------------------------- */
/* In a polyploid a guide's near copies are mostly the gene's own homeologs.  With the family genes of its arena on
 * the handle, the handle says which of them a candidate site cuts in and gives every guide site a second row that
 * counts only the candidates of its own family, so the difference to the plain row is what lies outside the family.
 * The handle's PAM must be its pattern's last 3 letters (T = l + 3): a '+' site at forward start p cuts at p + l - 3,
 * a '-' site at forward start j cuts at j.
 *
 * Rows r = 0 .. n_rows - 1 are the family genes that have a range in this arena, in GFF order: the closed range
 * [lo, hi] of arena positions, a family id (any value but 0xFFFFFFFF, the same id on every handle of a genome) and the
 * gene's bit in its family's cover word (member < 64).  cover_mm (0 .. max_mm): a guide site within that many
 * mismatches covers the gene it cuts in.  Replaces earlier families; n_rows = 0 with lo = NULL takes them off.
 * Adds 4 (max_mm + 1) + 24 bytes per candidate and 24 per row to the handle, counted against its budget
 * (CRP_ERR_CAPACITY).  CRP_ERR_INVALID with a crp_last_error text: another PAM geometry, cover_mm outside 0 .. max_mm,
 * a member bit of 64 or more, family id 0xFFFFFFFF. */
int crp_search_self_set_families(crp_search_self *self, const uint32_t *lo, const uint32_t *hi, const uint32_t *family,
                                 const uint32_t *member, uint64_t n_rows, int cover_mm);
/* Lowers the pairs one family compare launch covers and the smallest slice of a member's run (0: the defaults, 2^36
 * and 2 048; a slice has at least 8 candidates).  Results do not depend on either. */
int crp_search_self_family_set_limits(crp_search_self *self, uint64_t pairs_per_launch, uint32_t slice_min);
/* Owner and family of every candidate: the owner is the smallest row whose range holds the site's cut.  Zeroes the
 * family rows; a guide site's cover word starts with its owner's bit.  CRP_ERR_STATE without families. */
int crp_search_self_family_assign(crp_search_self *self);
/* The guide sites of `guides` that have an owner against the candidates of `candidates` that have an owner of the same
 * family, all pairs, compared and valued as crp_search_self_compare does (the guides handle's scheme state and
 * max_mm); adds into the family rows of `guides`.  Once per ordered pair of handles, after both were assigned
 * (CRP_ERR_STATE otherwise); it needs no ordering. */
int crp_search_self_family_compare(crp_search_self *guides, crp_search_self *candidates);
/* The family rows of the guide sites, in the order of crp_search_self_fetch: the owner's row (0xFFFFFFFF: none), its
 * family id (0xFFFFFFFF: none), fam_counts (max_mm + 1 per site: the candidates of the same family at k mismatches,
 * the site itself not counted), fam_sum (their values) and fam_cover (bit m: the site cuts in member m, or a guide
 * site that cuts in member m lies within cover_mm).  Any pointer may be NULL. */
int crp_search_self_family_fetch(crp_search_self *self, uint32_t *owner, uint32_t *family, uint32_t *counts, uint64_t *sum,
                                 uint64_t *cover, uint64_t cap);
/* The family rows handed to the hits of the arena's last scan, as crp_search_self_join_hits hands the plain rows (the
 * same sites join): counts, sum, cover and family id per hit of the '+' and the '-' table.  An unjoined hit gets
 * all-ones counts and sum, cover 0 and family 0xFFFFFFFF; a joined hit without a family zeros and family 0xFFFFFFFF. */
int crp_search_self_family_join_hits(crp_search_self *self, int guide_len, uint32_t *counts_plus, uint64_t *sum_plus,
                                     uint64_t *cover_plus, uint32_t *family_plus, uint32_t *counts_minus, uint64_t *sum_minus,
                                     uint64_t *cover_minus, uint32_t *family_minus);
/* out[0] ms of the bounds and assign kernels, out[1] ms of family compare kernels, out[2] pairs compared, out[3]
 * family compare launches, out[4] device bytes the families add, out[5] ms of the family join.  n <= 6. */
int crp_search_self_family_stats(const crp_search_self *self, double *out, int n);

/* ---- guide selection: the best K guides of every gene -------------------------------- */
/* The gene rows of an annotation (type `gene`, file order): index of the seqid (crp_annotation_seqid), start and end
 * as the GFF gives them (1-based, closed), and the labels "gene:<ident>" -- without the annotation_info suffix -- back
 * to back in label_blob with n_genes + 1 offsets.  n_genes is crp_annotation_stats'; *label_bytes the blob's size.
 * Any pointer may be NULL. */
int crp_annotation_genes(const crp_annotation *an, uint64_t *seqid, int64_t *start, int64_t *end, uint8_t *label_blob,
                         uint64_t *label_off, uint64_t *label_bytes);
/* The genes of the texts of one arena, in arena positions: entries and dec as crp_annotation_track takes them (the
 * same mapping: string index = coordinate + dec - 1 - first, plus the text's arena offset), each gene's range clipped
 * to the text.  One row per (text, gene of its seqid) that keeps at least one position, texts in arena order, genes
 * in file order: lo[], hi[] (closed) and gene[], the gene's index in crp_annotation_genes.  A gene with start > end,
 * with a seqid no text names or outside its text has no row.  Capacity protocol as crp_annotation_track. */
int crp_annotation_gene_layout(const crp_annotation *an, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *lo,
                               uint32_t *hi, uint64_t *gene, uint64_t cap, uint64_t *n_out);
/* One byte per label-set string (crp_annotation_stats' n_strings): 1 when the set holds a CDS label. */
int crp_annotation_cds_flags(const crp_annotation *an, uint8_t *flags);

/* A segmented top-K over the hit tables of an arena's last crp_scan_score at guide length 20.  Gene g is the closed
 * range [lo[g], hi[g]] of arena positions.  A row has a cut site when its score is not -1: match index i - 3 on the
 * '+' table, j on the '-' table (as crp_annotate_lookup).  It is IN gene g when lo[g] <= cut site <= hi[g], and it
 * PASSES when also
 *   score >= min_score                                                          (float64)
 *   with a self-search handle: counts[0] != 0xFFFFFFFF (joined), counts[0] <= max_mm0 and hit_sum <= max_hit_sum
 *   with require_cds: the flag of its label-set id is non-zero (CRP_NO_FEATURE fails)
 *   with property limits (crp_select_set_property_limits) and with repair limits (crp_select_set_repair_limits): those hold
 * Passing rows are ordered by higher score (as its 64 bits, unsigned), then smaller cut site, then '+' before '-': a
 * total order, so the result does not depend on how the work is cut.  Per gene: n_in (rows in it), n_pass (passing
 * rows) and sel[g * K .. g * K + K): the first min(K, n_pass) passing rows as row index | strand << 31, 0xFFFFFFFF
 * beyond.  Genes may overlap or repeat; each is selected for on its own. */
typedef struct crp_select crp_select;
typedef struct crp_select_params {
    double min_score;
    uint64_t max_hit_sum; /* read with a self-search handle only */
    uint32_t max_mm0;     /* read with a self-search handle only */
    int32_t k;            /* 1 .. CRP_SELECT_MAX_K */
    int32_t require_cds;
    int32_t reserved;
} crp_select_params;
#define CRP_SELECT_MAX_K 64
#define CRP_SELECT_DEFAULT_SLICE_ROWS 65536
#define CRP_SELECT_MIN_SLICE_ROWS 64
#define CRP_SELECT_NONE 0xFFFFFFFFu
/* lo / hi: n_genes closed ranges, lo <= hi < 2^31 (CRP_ERR_INVALID otherwise); CRP_ERR_STATE: arena not sealed.  The
 * arena must outlive the handle. */
int crp_select_create(crp_arena *arena, const uint32_t *lo, const uint32_t *hi, uint64_t n_genes, crp_select **out);
int crp_select_destroy(crp_select *select);
/* The CDS flag of every label-set id (crp_annotation_cds_flags), for require_cds. */
int crp_select_set_flags(crp_select *select, const uint8_t *flags, uint64_t n_flags);
/* A gene's rows are cut into work items of at most slice_rows rows, one wave each (0 = the default, 65 536; at
 * least 64); one launch covers at most 2^20 items.  Results do not depend on it. */
int crp_select_set_limits(crp_select *select, uint64_t slice_rows);
/* self: NULL, or the self-search handle of the same arena after its crp_search_self_join_hits on the current tables.
 * CRP_ERR_STATE with a crp_last_error text: no hit tables of guide length 20, require_cds without flags or without
 * the ids of a crp_annotate_lookup on the current tables, a handle that has not joined.  CRP_ERR_INVALID: k out of
 * range, a min_score that is NaN, a handle of another arena. */
int crp_select_run(crp_select *select, const crp_select_params *params, crp_search_self *self);
/* The results of the last run (CRP_ERR_STATE without one): n_in and n_pass (n_genes each) and sel (n_genes * k).
 * Any pointer may be NULL. */
int crp_select_fetch(crp_select *select, uint32_t *n_in, uint32_t *n_pass, uint32_t *sel);
/* Measurement of the last run: out[0] ms of the bounds kernel, out[1] ms of the select launches, out[2] ms of the
 * merge launches (HIP events), out[3] work items, out[4] select launches, out[5] the longest select launch in ms,
 * out[6] table rows the items cover, out[7] bytes read per such row, out[8] genes that went through the merge.
 * n: how many of these to write (<= 9). */
int crp_select_stats(const crp_select *select, double *out, int n);
/* Property limits (the column of crp_guide_properties, below): with limits set a row PASSES only if also
 * gc_min <= gc <= gc_max, run <= max_run, t_run <= max_t_run and stem <= max_stem; crp_select_run then reads 4 more
 * bytes per row (crp_select_stats counts them) and returns CRP_ERR_STATE when the arena holds no property column for its
 * current tables.  NULL clears the limits. */
typedef struct crp_select_property_limits {
    uint32_t gc_min, gc_max, max_run, max_t_run, max_stem;
} crp_select_property_limits;
int crp_select_set_property_limits(crp_select *select, const crp_select_property_limits *limits);

/* ---- guide sequence properties (opt-in, absent from the reference) --------------------- */
/* After crp_scan_score on `arena` at guide length l = 1 .. 50: four values per kept hit, each a pure function of the l
 * letters of its guide WINDOW in the forward text -- s[i - l : i] for a '+' row with match index i, s[j + 3 : j + 3 + l]
 * for a '-' row with match index j.  A window letter is a BASE when it is one of acgtACGT or U (case is ignored, U is A);
 * everything else -- N, IUPAC letters, decoration, positions past the end of the contig string (a '-' row may have up
 * to 10) -- is a non-base.
 *   gc      window letters that are C or G
 *   run     the longest run of equal bases (a non-base ends a run; 0 when the window holds no base)
 *   t_run   the longest run of T in the spacer's own orientation: of T in a '+' window, of A in a '-' window (whose
 *           spacer is the window's reverse complement)
 *   stem    the largest s >= 0 for which indices a, b exist with w[a + t] complementary to w[b - t] (A-T or C-G, both
 *           bases, no wobble pair) for t = 0 .. s - 1 and (b - s + 1) - (a + s) >= 3: at least three unpaired letters
 *           in the loop.  At most (l - 3) / 2; the same for a window and its reverse complement.
 * One uint32 per row: gc | run << 8 | t_run << 16 | stem << 24, table order.  The column stays in HBM until the arena's
 * next scan (crp_select_set_property_limits reads it there) and is copied to props_plus / props_minus (n_plus / n_minus
 * values; either may be NULL).  One kernel lane per row, one launch for both tables.  CRP_ERR_STATE: no tables;
 * CRP_ERR_INVALID with a crp_last_error text: the tables were scanned at guide length 0. */
int crp_guide_properties(crp_arena *arena, uint32_t *props_plus, uint32_t *props_minus);
/* The last crp_guide_properties of the arena (CRP_ERR_STATE without a column for the current tables): out[0] ms of its
 * kernel (HIP events), out[1] rows, out[2] the guide length.  n: how many of these to write (<= 3).  With
 * crp_profile_enable(ctx, 2) the kernel is also accounted under CRP_K_PROPERTIES. */
int crp_guide_properties_stats(const crp_arena *arena, double *out, int n);

/* ---- repair outcome of the cut (opt-in, absent from the reference) ---------------------- */
/* After crp_scan_score on `arena` (any guide length; it is not used): what microhomology-mediated end joining is
 * predicted to leave behind at the cut of every kept hit, after Bae, Kweon, Kim and Kim 2014 -- two integers per row,
 * each a pure function of the 2 * flank letters around the cut in the forward text.
 *   cut      the boundary c between s[c - 1] and s[c]: c = i - 3 for a '+' row with match index i, c = j + 6 for a '-' row
 *            with match index j -- three letters into the protospacer from the PAM on either strand.  (NOT the CSV's
 *            `cutsite` column, which for '-' rows is the reference's end_pos - 3 = j.)
 *   window   w[p] = s[c - flank + p], p = 0 .. 2 flank - 1.  A letter is a BASE when it is one of acgtACGT or U (case is
 *            ignored, U is A); N, IUPAC letters, decoration, positions outside the contig string are non-bases.
 *   n_d      for a deletion length d = 1 .. 2 flank - 1: over every maximal run, of length k >= 2, of p in
 *            [max(0, flank - d), min(flank, 2 flank - d)) with w[p] == w[p + d], both bases: k + (its letters that are C or G)
 *   mh       sum over d of W[d] n_d, W[d] = floor(1000 exp(-d / 20) + 1/2) (csrc/microhomology_weights.def)
 *   oof      the same sum over the d that are no multiple of 3
 * One uint64 per row: mh | oof << 32 (both below 2^20), table order; 0 for a window without a microhomology.  The
 * published quantities are mh / 10 (microhomology score) and 100 oof / mh (out-of-frame score).  The column stays in HBM
 * until the arena's next scan (crp_select_set_repair_limits reads it there) and is copied to plus / minus (n_plus /
 * n_minus values; either may be NULL).  One kernel lane per row, one launch for both tables; empty tables are fine.
 * CRP_ERR_INVALID with a crp_last_error text: flank outside 2 .. 32; CRP_ERR_STATE: no tables. */
int crp_repair_scores(crp_arena *arena, int flank, uint64_t *plus, uint64_t *minus);
/* The last crp_repair_scores of the arena (CRP_ERR_STATE without a column for the current tables): out[0] ms of its
 * kernel (HIP events), out[1] rows, out[2] the flank.  n: how many of these to write (<= 3). */
int crp_repair_scores_stats(const crp_arena *arena, double *out, int n);
/* Repair limits of a selection (the column of crp_repair_scores): with limits set a row PASSES only if also
 * mh >= min_mh (tenths of the microhomology score) and 100 oof >= min_oof_pct mh (min_oof_pct 0 .. 100, else
 * CRP_ERR_INVALID); with min_oof_pct > 0 a row with mh = 0, which has no out-of-frame score, fails.  crp_select_run then
 * reads 8 more bytes per row (crp_select_stats counts them) and returns CRP_ERR_STATE when the arena holds no repair
 * column for its current tables.  NULL clears the limits. */
typedef struct crp_select_repair_limits {
    uint32_t min_mh, min_oof_pct;
} crp_select_repair_limits;
int crp_select_set_repair_limits(crp_select *select, const crp_select_repair_limits *limits);

/* ---- guide pairs: the best KP deletion pairs of every gene (opt-in) --------------------- */
/* Two guides in one array cut out the piece between them.  On a crp_select handle, over the same tables and genes:
 *   eligible   the rows that PASS for gene g (crp_select_run's rule and predicate, unchanged)
 *   boundary   c of a row, as crp_repair_scores defines it: i - 3 for a '+' row, j + 6 for a '-' row (NOT the cut site
 *              that decides membership, nor the CSV's `cutsite`)
 *   pair       (a, b): two eligible rows of one gene with c_a < c_b; D = c_b - c_a is the deletion's length, the letters
 *              s[c_a : c_b) go
 *   qualifies  dmin <= D <= dmax; with frameshift, D mod 3 != 0; and bit sa * 2 + sb of orientation_mask is set (s = 0
 *              for '+', 1 for '-': 0xF any, 4 PAM-out = '-' left and '+' right, 2 PAM-in)
 *   order      higher min(score_a, score_b) (the doubles' bits, unsigned), then higher max, then smaller c_a, then
 *              smaller c_b, then smaller sa * 2 + sb: total
 * Per gene: n_pass (eligible rows), n_pairs (all qualifying pairs, 64 bits) and pairs[g * KP * 2 ..): the first
 * min(KP, n_pairs) pairs in that order, each as a then b in sel's packing (row | strand << 31), 0xFFFFFFFF beyond.
 * Pairs may share a guide. */
typedef struct crp_select_pair_params {
    int32_t k;                 /* KP: 1 .. CRP_SELECT_PAIRS_MAX_K, independent of crp_select_params.k (which is not read) */
    uint32_t dmin, dmax;       /* 1 <= dmin <= dmax <= CRP_SELECT_PAIRS_MAX_DISTANCE */
    uint32_t orientation_mask; /* 1 .. 15 */
    int32_t frameshift;
} crp_select_pair_params;
#define CRP_SELECT_PAIRS_MAX_K 64
#define CRP_SELECT_PAIRS_MAX_DISTANCE 65535
#define CRP_SELECT_DEFAULT_PAIR_SLICE_ROWS 1024
#define CRP_SELECT_MIN_PAIR_SLICE_ROWS 64
/* A gene's a-rows are cut into work items of at most pair_slice_rows rows, one wave each (0 = the default, 1 024; at
 * least 64): a limit of its own, since an item costs rows x partners.  Results do not depend on it. */
int crp_select_set_pair_limits(crp_select *select, uint64_t pair_slice_rows);
/* Prerequisites and error codes as crp_select_run (params: its thresholds; params->k is not read).  CRP_ERR_INVALID
 * with a crp_last_error text: KP outside 1 .. 64, dmin = 0, dmin > dmax, dmax > 65 535, a mask that is 0 or above 15.
 * Leaves the results of crp_select_run alone. */
int crp_select_run_pairs(crp_select *select, const crp_select_params *params, const crp_select_pair_params *pair_params,
                         crp_search_self *self);
/* The results of the last crp_select_run_pairs (CRP_ERR_STATE without one): n_pass and n_pairs (n_genes each) and pairs
 * (n_genes * KP * 2).  Any pointer may be NULL. */
int crp_select_fetch_pairs(crp_select *select, uint32_t *n_pass, uint64_t *n_pairs, uint32_t *pairs);
/* Measurement of the last crp_select_run_pairs: out[0] ms of the pass-key kernel, out[1] ms of the pair launches,
 * out[2] ms of the merge launches (HIP events), out[3] work items, out[4] pair launches, out[5] the longest pair launch
 * in ms, out[6] pair evaluations (partner rows streamed), out[7] qualifying pairs.  n: how many to write (<= 8). */
int crp_select_pairs_stats(const crp_select *select, double *out, int n);

/* ---- distinct pairs: KP pairs per gene that share no guide (opt-in) ----------------------- */
/* crp_select_run_pairs ranks a gene's pairs one by one, and its best pairs may share one very good guide: constructs that
 * fail together when that guide fails.  Everything of the pair selection stands -- eligible rows, the boundary c, qualifying
 * pairs, the total order, n_pass and n_pairs.  New, per layout row g:
 *   distinct   walk the qualifying pairs of g in that order; take a pair iff NEITHER of its two rows is a row of a pair
 *              already taken; stop at KP taken.  (Round t takes the first qualifying pair in the order that has no row
 *              among the picks of rounds < t.)
 *   row        a table row of one strand, in sel's packing row | strand << 31: a '+' row at i and the '-' row at i - 9 have
 *              equal boundaries and are different guides.  A row taken as the left guide a of one pair shuts out the
 *              pairs that offer it as b, and the other way round.
 * Per gene: n_pass and n_pairs exactly as crp_select_run_pairs gives them, whatever the picks; n_distinct, the pairs
 * taken, at most min(KP, n_pairs, n_pass / 2); and pairs[g * KP * 2 ..) in pick order, which is the pairs' order,
 * 0xFFFFFFFF beyond n_distinct.  At KP = 1 the result is crp_select_run_pairs' at KP = 1 bit for bit.  Exact and
 * integer-only: the result does not depend on how the work was cut.  Greedy: the best pair is always taken, whatever it
 * shuts out; not a maximum-weight matching. */
/* Prerequisites, parameter checks, refusals and error codes are exactly crp_select_run_pairs' (one host function checks
 * both).  Genes are cut into items by crp_select_set_pair_limits' pair_slice_rows; a gene in one item runs all its rounds
 * in one launch, the others take a step launch and a pick launch a round: at most 2 KP + 3 launches per block of
 * items_per_launch items.  The run has buffers and results of its own: those of crp_select_run, _run_pairs, _run_spaced,
 * _run_self and the family step stay valid before and after it. */
int crp_select_run_pairs_distinct(crp_select *select, const crp_select_params *params, const crp_select_pair_params *pair_params,
                                  crp_search_self *self);
/* The results of the last crp_select_run_pairs_distinct (CRP_ERR_STATE without one): n_pass, n_pairs and n_distinct
 * (n_genes each) and pairs (n_genes * KP * 2).  Any pointer may be NULL. */
int crp_select_fetch_pairs_distinct(crp_select *select, uint32_t *n_pass, uint64_t *n_pairs, uint32_t *n_distinct, uint32_t *pairs);
/* Measurement of the last crp_select_run_pairs_distinct: out[0] ms of the pass-key kernel, out[1] ms of the whole-gene item
 * launches, out[2] ms of the cut genes' step launches, out[3] ms of their pick launches (HIP events), out[4] host rounds,
 * out[5] kernel launches, out[6] the longest launch in ms, out[7] work items, out[8] cut genes, out[9] partner rows
 * streamed, summed over all rounds, out[10] pairs taken, out[11] qualifying pairs.  n: how many to write (<= 12). */
int crp_select_pairs_distinct_stats(const crp_select *select, double *out, int n);
/* At most items_per_launch work items per launch of the distinct pair run (0 = the default and the most, 2^20; more:
 * CRP_ERR_INVALID).  Results do not depend on it. */
int crp_select_set_pair_distinct_limits(crp_select *select, uint64_t items_per_launch);

/* ---- spaced selection: K guides per gene whose cut sites lie at least D apart (opt-in) --- */
/* crp_select_run's K best rows of a gene cluster: a good 30-mer context lifts its neighbours.  On a crp_select handle,
 * over the same tables and genes, per layout row g:
 *   passing    the rows that PASS for gene g: exactly those crp_select_run counts in n_pass[g] under the handle's flags,
 *              property, repair and variant limits
 *   order      crp_select_run's: higher score bits (unsigned 64-bit), then smaller cut site, then '+' before '-'; the
 *              cut site is i - 3 for a '+' row and j for a '-' row (NOT the pairs' cut boundary)
 *   spaced     walk the passing rows of g in that order; take a row iff |cut - cut(p)| >= min_distance for EVERY row p
 *              already taken; stop at K taken.  (Round t takes the best passing row that is not within
 *              min_distance - 1 of any earlier pick.)
 * Per gene: n_pass (as crp_select_run's, whatever the distance), n_spaced (the rows taken, at most min(K, n_pass)) and
 * sel[g * K ..): the rows taken in pick order, in crp_select_run's packing (row | strand << 31), 0xFFFFFFFF beyond
 * n_spaced.  Exact and integer-only: the result does not depend on how the work was cut.  min_distance = 0 is
 * crp_select_run's sel bit for bit; 1 forbids only equal cut sites.  Greedy by score, not a maximum-weight spread. */
#define CRP_SELECT_MAX_SPACING 0x7FFFFFFFu
/* Prerequisites and their error codes as crp_select_run (params: its thresholds and K).  CRP_ERR_INVALID with a
 * crp_last_error text: K outside 1 .. 64, min_distance > CRP_SELECT_MAX_SPACING, and coding, edit, splice or family
 * limits in force on the handle (their kernels own a predicate per gene and row; the spaced rounds read one key per
 * row).  Genes are cut into items by crp_select_set_limits' slice_rows; a gene in one item runs all its rounds in one
 * launch, the others take a step launch and a pick launch a round: at most 2 K + 3 launches per 2^20 items.  Leaves
 * the results of crp_select_run and crp_select_run_pairs alone. */
int crp_select_run_spaced(crp_select *select, const crp_select_params *params, uint32_t min_distance, crp_search_self *self);
/* The results of the last crp_select_run_spaced (CRP_ERR_STATE without one): n_pass and n_spaced (n_genes each) and sel
 * (n_genes * K).  Any pointer may be NULL. */
int crp_select_fetch_spaced(crp_select *select, uint32_t *n_pass, uint32_t *n_spaced, uint32_t *sel);
/* Measurement of the last crp_select_run_spaced: out[0] ms of the pass-key kernel, out[1] ms of the whole-gene item
 * launches, out[2] ms of the cut genes' step launches, out[3] ms of their pick launches (HIP events), out[4] host rounds,
 * out[5] kernel launches, out[6] the longest launch in ms, out[7] work items, out[8] cut genes.  n: how many to write
 * (<= 9). */
int crp_select_spaced_stats(const crp_select *select, double *out, int n);

/* ---- self selection: the K most specific guide sites of every gene, for any nuclease (opt-in) --- */
/* crp_select_run ranks the rows of the NGG scan by their on-target score.  This run ranks the rows of a self-search handle
 * (crp_search_self_*: any pattern of up to 32 letters, the PAM on either side) by their specificity, where they lie in HBM.
 * It reads no scan tables.  Per arena, on a crp_select handle (its genes lo[] / hi[], its flags, its slice_rows), with a
 * handle of T pattern letters, P PAM letters, G = T - P guide-region letters and M mismatches:
 *   cut letter  of a guide site with forward start s, for a cut offset c (1 <= c <= T - 1, in pattern coordinates: the cut
 *               lies before pattern position c of the oriented window): s + c on '+', s + T - c on '-'.  With ...NGG (T = 23)
 *               and c = 17 a '+' site's cut letter is crp_select_run's i - 3; the '-' rule is the true mirror, j + 6, where
 *               crp_select_run keeps the reference's j
 *   in          only guide sites count (a candidate that is no guide site is ignored): in gene g when lo <= cut <= hi
 *   passes      counts[0] <= max_mm0; on a scored handle hit_sum <= max_hit_sum; with require_cds the flag byte
 *               (crp_select_set_flags) of the label-set id of the track interval (crp_annotate_set_track) under the cut
 *               letter is non-zero; gc_min <= GC letters of the guide region <= gc_max; the longest run of T in the guide
 *               region <= max_t_run
 *   order       smaller e first, then the smaller cut letter, then '+' before '-'.  Scored handle: e = hit_sum +
 *               ((uint64)counts[0] << 30), a perfect copy elsewhere weighing like a hit of full value.  Unscored handle: e =
 *               min(counts[0], 65 535) << 48 | min(counts[j], 4 095) << (48 - 12 j) for j = 1 .. M
 *   result      per gene: n_in (guide sites in the gene), n_pass (passing ones) and sel[g * K ..): the first min(K, n_pass)
 *               passing sites in that order, each as its candidate index in extraction order, 0xFFFFFFFF beyond
 * Exact and integer-only: the result does not depend on how the work was cut. */
typedef struct crp_select_self_params {
    uint64_t max_hit_sum; /* 0xFFFFFFFFFFFFFFFF: no bound; not read on an unscored handle */
    uint32_t max_mm0;     /* 0xFFFFFFFF: no bound */
    int32_t k;            /* 1 .. CRP_SELECT_MAX_K */
    int32_t cut_offset;   /* c: 1 .. T - 1 */
    int32_t require_cds;
    uint32_t gc_min, gc_max; /* counts of letters; 0 and 0xFFFFFFFF: no bound */
    uint32_t max_t_run;      /* 0xFFFFFFFF: no bound */
    uint32_t reserved;
} crp_select_self_params;
/* The run.  CRP_ERR_INVALID with a crp_last_error text: K outside 1 .. 64, c outside 1 .. T - 1, gc_min > gc_max, a handle of
 * another arena.  CRP_ERR_STATE: a handle that has not been the query of a crp_search_self_compare on every segment 0 .. M
 * (with several arenas the caller compares it against every arena's handle: only "at least once per segment" is tracked),
 * require_cds without crp_select_set_flags or without a track on the arena.  CRP_ERR_UNSUPPORTED: more than 2^32 - 2
 * candidates.  Genes are cut into items by crp_select_set_limits' slice_rows, at most crp_select_set_self_limits'
 * items a launch; cut genes are merged by crp_select_run's merge.  Leaves the results of the handle's other runs alone. */
int crp_select_run_self(crp_select *select, const crp_select_self_params *params, crp_search_self *self);
/* Work items per launch of crp_select_run_self (0: the default, 2^20; more is CRP_ERR_INVALID).  Results do not depend on it;
 * tests lower it to put a cut gene's items on both sides of a launch boundary. */
int crp_select_set_self_limits(crp_select *select, uint64_t items_per_launch);
/* The results of the last crp_select_run_self (CRP_ERR_STATE without one): n_in, n_pass (n_genes each), sel (n_genes * K), and
 * of the selected candidates, entry by entry beside sel (gathered on the device: K rows a gene are copied, never a column):
 * arena_pos (forward start), strand (0 '+', 1 '-'), hi, lo (the oriented window's code bits), counts (M + 1 each) and
 * hit_sum (all-ones on an unscored handle).  All-ones where sel has no candidate.  Any pointer may be NULL. */
int crp_select_fetch_self(crp_select *select, uint32_t *n_in, uint32_t *n_pass, uint32_t *sel, uint32_t *arena_pos, uint8_t *strand,
                          uint32_t *hi, uint32_t *lo, uint32_t *counts, uint64_t *hit_sum);
/* Measurement of the last crp_select_run_self: out[0] ms of the bounds kernel, out[1] ms of the item launches, out[2] ms of the
 * merge launches, out[3] ms of the gather kernel (HIP events), out[4] item launches, out[5] work items, out[6] candidates
 * streamed (the runs' rows).  n: how many to write (<= 7). */
int crp_select_self_stats(const crp_select *select, double *out, int n);
/* The on-target model in the self selection.  Held on the select handle for its later
 * crp_select_run_self calls, which then refuse (CRP_ERR_STATE) a self-search handle whose model has not been run.
 *   has_min        a site passes only if it has a sum and the sum is >= min_sum (NaN min_sum: CRP_ERR_INVALID)
 *   rank_by_model  a site passes only if it has a sum, and the order is larger sum first, then the smaller cut letter, then
 *                  '+' before '-'.  The list key is computed from the bits b of the sum, -0.0 first replaced by +0.0:
 *                  b ^ 0x8000000000000000 for b >= 0 as a signed value, ~b otherwise
 * Every test of crp_select_run_self stays a filter.  With both 0 (the default) every result bit is what it is without a model. */
int crp_select_set_self_model(crp_select *select, int rank_by_model, int has_min, double min_sum);
/* Beside crp_select_fetch_self: the on-target sum of every selected candidate (n_genes * K), NaN where sel has no candidate,
 * where the site has no sum or where the handle's model had not been run. */
int crp_select_fetch_self_model(crp_select *select, double *model_sum);

/* ---- coding position: where in the coding sequence a guide cuts (opt-in) ---------------- */
/* crp_annotation_build also reads the `mRNA` / `transcript` rows, the Parent links and the gene rows' strand, and builds a
 * CODING MODEL of every gene (cropsr_amd/coding.py states the definition):
 *   transcripts  of gene G (non-empty ID): the mRNA / transcript rows on G's seqid with a Parent value equal to G's ID, each
 *                with the CDS rows on that seqid whose Parent names its ID; plus one implicit transcript of the CDS rows
 *                whose Parent names G itself.  Parent is a comma-separated list; links are resolved after the whole file is
 *                read; of several rows with one ID the first owns the children; CDS rows with start > end are dropped
 *   coding       the coding letters of a transcript are the union of its CDS rows' closed ranges (not clipped to the gene),
 *                L_T their number; a transcript without one is not counted.  n_tx = the coding transcripts
 *   primary P    the coding transcript with the largest L_T, on a tie the earlier row (the implicit one stands at the gene row)
 *   no model     a strand (column 7 of the gene row) other than + or -, n_tx = 0, or L_P above 2^32 - 1
 * Per gene of crp_annotation_genes: strand ('+', '-', or '.' for anything else), n_tx and L_P (both 0 without a model).  Any
 * pointer may be NULL. */
int crp_annotation_gene_coding(const crp_annotation *an, uint8_t *strand, uint32_t *n_tx, uint32_t *length);
/* The coding model in arena positions, beside crp_annotation_gene_layout: the same entries and dec give EXACTLY the same
 * rows in the same order.  Per row: info = n_tx | (strand '-') << 16 | (has a model) << 17, length = L_P, and first = the
 * index of its first step; its steps end where the next row's begin (the last row's at *n_steps).  A row's steps are a
 * function over the cut boundaries c of the arena (c lies between s[c - 1] and s[c]), clipped to the row's text:
 *   at[k]    ascending change points; before at[0] nothing holds, step k is at[k] <= c < at[k + 1]
 *   word[k]  cover (bits 0..15: the coding transcripts c is INSIDE -- s[c - 1] and s[c] both coding letters) |
 *            (inside P) << 16 | (s[c] is a coding letter of P) << 17
 *   cum[k]   P's coding letters with index below at[k], counted on the whole contig: inside step k the count below c is
 *            cum[k] + (bit 17) * (c - at[k])
 * A merged segment [a, b] contributes the change points a, a + 1 and b + 1; points that change nothing are left out.
 * Capacity protocol as crp_annotation_track, for the rows and the steps at once: CRP_ERR_CAPACITY with the needed sizes in
 * *n_rows / *n_steps.  CRP_ERR_UNSUPPORTED: a gene with more than 65 535 coding transcripts. */
int crp_annotation_coding_layout(const crp_annotation *an, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *info,
                                 uint32_t *length, uint64_t *first, uint64_t cap_rows, uint64_t *n_rows, uint32_t *at, uint32_t *word,
                                 uint32_t *cum, uint64_t cap_steps, uint64_t *n_steps);
/* The model of a crp_select handle: the arrays of crp_annotation_coding_layout for its genes, first with n_rows + 1
 * elements (the last one n_steps).  CRP_ERR_INVALID with a crp_last_error text: n_rows is not the handle's n_genes, first
 * does not ascend to n_steps, a row's change points do not ascend.  n_rows = 0 with NULL arrays clears the model. */
int crp_select_set_coding(crp_select *select, const uint32_t *info, const uint32_t *length, const uint64_t *first, uint64_t n_rows,
                          const uint32_t *at, const uint32_t *word, const uint32_t *cum, uint64_t n_steps);
/* Coding limits: with limits set a row PASSES for gene g only if also g has a model, the row's cut -- the boundary c of
 * crp_repair_scores, i - 3 on the '+' table and j + 6 on the '-' table, NOT the cut site that decides membership -- is
 * inside P, min_pct L_P <= 100 off <= max_pct L_P and 100 cover >= min_transcripts_pct n_tx (64-bit integer products),
 * where off = P's coding letters 5' of the cut in the gene's orientation: cum_P(c) for a '+' gene, L_P - cum_P(c) for a
 * '-' gene.  Percentages 0 .. 100 with min_pct <= max_pct, else CRP_ERR_INVALID.  NULL clears the limits.  With limits
 * and no model crp_select_run returns CRP_ERR_STATE; crp_select_run_pairs refuses coding limits (CRP_ERR_UNSUPPORTED):
 * its eligibility key is per table row, not per gene. */
typedef struct crp_select_coding_limits {
    uint32_t min_pct, max_pct, min_transcripts_pct;
} crp_select_coding_limits;
int crp_select_set_coding_limits(crp_select *select, const crp_select_coding_limits *limits);
/* off[q] and cover[q] of n queries (gene_row[q]: a gene of the handle; packed_row[q]: a table row in sel's packing, row |
 * strand << 31), one kernel lane each; off = 0xFFFFFFFF where the cut is not inside P.  Needs the model and the arena's
 * current tables, no limits and no run.  CRP_ERR_INVALID with a crp_last_error text: a gene or a row out of range
 * (checked on the host; nothing is launched).  CRP_ERR_STATE: no model, no tables. */
int crp_select_coding_eval(crp_select *select, const uint32_t *gene_row, const uint32_t *packed_row, uint64_t n, uint32_t *off,
                           uint32_t *cover);
/* out[0] ms of the select launches of the last crp_select_run that had coding limits (0: none), out[1] ms of the last
 * crp_select_coding_eval's kernel (HIP events), out[2] the steps of the model.  n: how many to write (<= 3). */
int crp_select_coding_stats(const crp_select *select, double *out, int n);

/* ---- base editing: guides that write a stop codon (opt-in) ------------------------------ */
/* A cytosine base editor makes no cut: it converts the C's of a small window of the protospacer (cropsr_amd/baseedit.py
 * states the definition).  Of a row of the hit tables after a scan at guide length 20:
 *   window   protospacer positions lo .. hi counted from the PAM-distal end, 1 <= lo <= hi <= 20; letter p is the arena
 *            position i - 21 + p of a '+' row (match index i) and j + 23 - p of a '-' row
 *   targets  the window's letters that are base C ('+' row) or base G ('-' row): they become T resp. A.  A base has its
 *            `ac` bit set, its code is (hi, lo); case is not read; positions outside the planes are non-bases, never read
 *   stops    relative to gene g with a model (crp_select_set_coding): the codons of the primary transcript P -- three
 *            adjacent arena positions, all bases, coding letters of P with indices 3 q, 3 q + 1, 3 q + 2 in the gene's
 *            orientation -- that are no stop and become TAA, TAG or TGA when every target among their letters is converted
 *   stop_off 3 q of the one with the smallest q, 0xFFFFFFFF if there is none; a gene without a model has stops = 0
 * Edit limits: with limits set a row PASSES for gene g only if also the edit writes a stop, min_pct L_P <= 100 stop_off <=
 * max_pct L_P (64-bit integer products) and targets <= max_targets.  window NULL: 4 .. 8.  limits NULL clears the limits.
 * CRP_ERR_INVALID with a crp_last_error text: a window out of range, a percentage above 100, min_pct > max_pct.  With edit
 * limits crp_select_run needs the model (CRP_ERR_STATE without) and refuses coding limits set at the same time
 * (CRP_ERR_UNSUPPORTED: one kernel per predicate); crp_select_run_pairs refuses edit limits (CRP_ERR_UNSUPPORTED). */
typedef struct crp_select_edit_window {
    uint32_t lo, hi;
} crp_select_edit_window;
typedef struct crp_select_edit_limits {
    uint32_t min_pct, max_pct, max_targets;
} crp_select_edit_limits;
int crp_select_set_edit_limits(crp_select *select, const crp_select_edit_window *window, const crp_select_edit_limits *limits);
/* counts[q] = targets | stops << 8 and stop_off[q] of n queries (gene_row[q]: a gene of the handle; packed_row[q]: a table
 * row in sel's packing), one kernel lane each.  Needs the model and the arena's current tables of guide length 20, no
 * limits and no run.  CRP_ERR_INVALID with a crp_last_error text: a window, a gene or a row out of range (checked on the
 * host; nothing is launched).  CRP_ERR_STATE: no model, no tables, tables of another guide length. */
int crp_select_edit_eval(crp_select *select, const crp_select_edit_window *window, const uint32_t *gene_row, const uint32_t *packed_row,
                         uint64_t n, uint32_t *counts, uint32_t *stop_off);
/* out[0] ms of the select launches of the last crp_select_run that had edit limits (0: none), out[1] ms of the last
 * crp_select_edit_eval's kernel (HIP events), out[2] the letters of the window last used.  n: how many to write (<= 3). */
int crp_select_edit_stats(const crp_select *select, double *out, int n);

/* ---- base editing: guides that destroy a splice site (opt-in) ---------------------------- */
/* Both base-editor families can knock a gene out without a stop codon: by changing a letter of the canonical GT that opens
 * an intron of the coding transcript or of the AG that closes it (cropsr_amd/baseedit.py states the definition).  Rows,
 * window, letters and the model are those of the section above.
 *   editor    CRP_EDITOR_CBE: the window's base C on a '+' row, base G on a '-' row; CRP_EDITOR_ABE: base A resp. base T
 *   targets   their number, 0 .. 20; it depends on no gene
 *   introns   relative to gene g with a model: in ascending positions an intron of the primary transcript P starts at a
 *             boundary x where x - 1 is a coding letter of P, x is not and cum_P(x) < L_P, and ends at x' where x' - 1 is
 *             not, x' is and cum_P(x') > 0; evidence comes from the steps inside the row's text alone
 *   sites     the letters x, x + 1 and x' - 2, x' - 1, evaluated when both are bases, both are no coding letters of P and
 *             they read GT resp. AG on a '+' gene (donor, acceptor), CT resp. AC on a '-' gene (acceptor, donor)
 *   destroyed an evaluated site with a target among its two letters; donors, acceptors: their numbers
 *   off       donor_off, acceptor_off: P's coding letters 5' of the intron of the destroyed site of that kind nearest the
 *             gene's 5' end (cum_P at its boundary, L_P - cum_P on a '-' gene), 1 .. L_P - 1; 0xFFFFFFFF without one
 * Splice limits: with limits set a row PASSES for gene g only if also, for a kind in `kinds`, off is not 0xFFFFFFFF and
 * min_pct L_P <= 100 off <= max_pct L_P (64-bit integer products), and targets <= max_targets.  With edit limits set as
 * well (CRP_EDITOR_CBE only) the two are alternatives: the row passes by either test under its own limits, both under the
 * window given here.  window NULL: 4 .. 8.  limits NULL clears the limits.
 * CRP_ERR_INVALID with a crp_last_error text: a window out of range, an unknown editor, a percentage above 100, min_pct >
 * max_pct, kinds outside 1 .. 3.  With splice limits crp_select_run needs the model (CRP_ERR_STATE without) and refuses
 * coding limits set at the same time and edit limits next to CRP_EDITOR_ABE (CRP_ERR_UNSUPPORTED); crp_select_run_pairs
 * refuses splice limits (CRP_ERR_UNSUPPORTED). */
#define CRP_EDITOR_CBE 0u
#define CRP_EDITOR_ABE 1u
#define CRP_SPLICE_DONOR 1u
#define CRP_SPLICE_ACCEPTOR 2u
typedef struct crp_select_splice_limits {
    uint32_t min_pct, max_pct, max_targets, kinds;
} crp_select_splice_limits;
int crp_select_set_splice_limits(crp_select *select, const crp_select_edit_window *window, uint32_t editor, const crp_select_splice_limits *limits);
/* counts[q] = targets | donors << 8 | acceptors << 16, off[2 q] = donor_off and off[2 q + 1] = acceptor_off of n queries
 * (gene_row[q]: a gene of the handle; packed_row[q]: a table row in sel's packing), one kernel lane each; off holds 2 n
 * words.  Needs the model and the arena's current tables of guide length 20, no limits and no run.  CRP_ERR_INVALID with a
 * crp_last_error text: a window, an editor, a gene or a row out of range (checked on the host; nothing is launched).
 * CRP_ERR_STATE: no model, no tables, tables of another guide length. */
int crp_select_splice_eval(crp_select *select, const crp_select_edit_window *window, uint32_t editor, const uint32_t *gene_row,
                           const uint32_t *packed_row, uint64_t n, uint32_t *counts, uint32_t *off);
/* out[0] ms of the select launches of the last crp_select_run that had splice limits (0: none), out[1] ms of the last
 * crp_select_splice_eval's kernel (HIP events), out[2] the letters of the window last used.  n: how many to write (<= 3). */
int crp_select_splice_stats(const crp_select *select, double *out, int n);

/* ---- gene families in the selection (opt-in) ------------------------------------------- */
/* Per gene of the handle (the rows of crp_select_create) its family id (0xFFFFFFFF: none; the ids of
 * crp_search_self_set_families) and the size of that family (1 for none).  For gene g with family f and a table row whose
 * joined site_family equals f (and is not none):
 *   outside_mm0 = counts[0] - fam_counts[0]   outside_hit_sum = hit_sum - fam_sum   members_hit = popcount(fam_cover)
 * and for every other row -- a gene in no family, a row that belongs to an overlapping gene of another family --
 *   outside_mm0 = counts[0]                   outside_hit_sum = hit_sum             members_hit = 1
 * n_genes must be the handle's; NULL, NULL, 0 takes the families off. */
int crp_select_set_family(crp_select *select, const uint32_t *gene_family, const uint32_t *family_size, uint64_t n_genes);
/* With limits a row passes crp_select_run for gene g only if, beyond the rest of the predicate, outside_mm0 <=
 * max_mm0_outside, outside_hit_sum <= max_hit_sum_outside (0xFFFFFFFF / 2^64 - 1: no bound) and members_hit >=
 * min_members, where CRP_SELECT_ALL_MEMBERS means the size of g's family.  The run then needs crp_select_set_family and a
 * self-search handle with both joins (CRP_ERR_STATE otherwise).  Not together with coding, edit or splice limits, and not
 * in crp_select_run_pairs (CRP_ERR_UNSUPPORTED): one kernel per predicate.  NULL clears the limits. */
#define CRP_SELECT_ALL_MEMBERS 0xFFFFFFFFu
typedef struct crp_select_family_limits {
    uint64_t max_hit_sum_outside;
    uint32_t max_mm0_outside, min_members;
} crp_select_family_limits;
int crp_select_set_family_limits(crp_select *select, const crp_select_family_limits *limits);
/* The four values of n queries (gene_row[q]: a gene of the handle; packed_row[q]: a table row in sel's packing), one kernel
 * lane each, from the joined columns of `self`, and fam_cover[q]: the row's cover word where the row's family is the
 * gene's (the members behind members_hit), 0 where it is not and the gene itself is the one member.  Needs crp_select_set_family and both joins on the arena's current tables,
 * no limits and no run.  CRP_ERR_INVALID with a crp_last_error text: a gene or a row out of range (checked on the host;
 * nothing is launched). */
int crp_select_family_eval(crp_select *select, crp_search_self *self, const uint32_t *gene_row, const uint32_t *packed_row, uint64_t n,
                           uint32_t *outside_mm0, uint64_t *outside_hit_sum, uint32_t *members_hit, uint32_t *family_size,
                           uint64_t *fam_cover);
/* out[0] ms of the select launches of the last crp_select_run that had family limits (0: none), out[1] ms of the last
 * crp_select_family_eval's kernel (HIP events).  n: how many to write (<= 2). */
int crp_select_family_stats(const crp_select *select, double *out, int n);

/* ---- family sets: the fewest guides that cut every member of a family (opt-in) ---------- */
/* A CANDIDATE of family f is a pair (gene g of the handle with family f, table row r) where r is in g and passes for g
 * exactly as crp_select_run counts n_pass for g with the handle's limits in force.  Its cover word is
 *   c = (site_family[r] == f ? fam_cover[r] : 0) | 1 << member(g)
 * and its gain against a word `covered` is popcount(c & ~covered).  One step picks, per family, the candidate of this
 * arena with the largest gain; ties go to the higher score (its 64 bits, unsigned), then to the smaller cut << 1 | strand,
 * then to the smaller gene row.  The greedy loop over the steps and the merge over the arenas are the caller's
 * (cropsr_amd/select.py, family_sets). */
#define CRP_FAMILY_SET_MAX_STEPS 64
/* The member bit (0 .. 63) of every gene of the handle in its family's cover word (0 for a gene in no family).  Needs
 * crp_select_set_family (CRP_ERR_STATE), which also clears the bits again; n_genes must be the handle's; NULL, 0 clears. */
int crp_select_set_family_members(crp_select *select, const uint32_t *gene_member, uint64_t n_genes);
/* gain 0: the family has no candidate in this arena that covers a new member (the other fields then mean nothing).  key:
 * the score's bits; cover: c; tie: cut << 1 | strand; row: table row | strand << 31 (sel's packing); gene: the handle's row. */
typedef struct crp_family_step_best {
    uint64_t key, cover;
    uint32_t gain, tie, row, gene;
} crp_family_step_best;
/* One step: best[f] for every family id f < n_families against covered[f] (host arrays).  params as crp_select_run takes
 * them (k is not read).  The plan -- bounds, work items, the family -> item list -- is built by the first call and kept
 * while the handle's families, slice_rows, the tables' sizes and params stay what they were: a later call launches the
 * step kernel and the pick kernel and nothing else.  CRP_ERR_STATE with a crp_last_error text: no crp_select_set_family, no
 * crp_select_set_family_members, no self-search handle with both joins on the current tables.  CRP_ERR_UNSUPPORTED: coding,
 * edit or splice limits are set (one kernel per predicate).  CRP_ERR_INVALID: a handle of another arena, a min_score that
 * is not a number, a gene whose family id is not below n_families. */
int crp_select_family_step(crp_select *select, const crp_select_params *params, crp_search_self *self, const uint64_t *covered,
                           uint64_t n_families, crp_family_step_best *best);
/* Of the last crp_select_family_step: out[0] ms of its step launches, out[1] ms of its pick launch (HIP events), out[2] its
 * work items, out[3] the table rows they cover, out[4] the bytes read per row; out[5] the plans built on this handle so far.
 * n: how many to write (<= 6). */
int crp_select_family_step_stats(const crp_select *select, double *out, int n);

/* ---- variant-aware guides: cultivar variants under every target site (opt-in) ------------- */
/* The guides are scanned from a reference assembly; the plant that is transformed carries SNPs and indels against it.
 * Per kept hit: how many variants of a VCF touch its target site, its guide, its PAM-proximal seed and its PAM.
 *
 * VARIANT INTERVALS.  For every VCF record and every kept ALT allele: strip the common prefix of REF and ALT (letters
 * compared without case), then the common suffix of what is left: REF', ALT' and p, the 1-based coordinate of the first
 * letter after the stripped prefix.  The allele is the closed interval [s, e] of contig coordinates, s = p,
 * e = p + len(REF') - 1.  A pure insertion (REF' empty) is [p, p - 1]: an empty interval at the junction between p - 1
 * and p.  An allele with REF' and ALT' both empty is dropped.  Always e >= s - 1.
 *
 * ARENA LAYOUT.  entries and dec as crp_annotation_track takes them, the first value of an entry being the index of the
 * text's CHROM among crp_variants_chrom's (any value >= their number: the text has no variants; a CHROM names a contig
 * when it equals its FASTA name exactly).  Coordinate c has string index c + dec - 1; inside a text that begins at
 * string index `first`, has `length` characters and lies at arena offset `offset` it has arena position index - first +
 * offset.  An interval is clipped to the text in string indices: s' = max(s, first), e' = min(e, first + length - 1); it
 * is kept when e' >= s' - 1.  Equal (s', e') pairs of one arena count once (a multi-allelic SNP is one variant).  The
 * track of an arena is two uint32 arrays of one length n, EACH ASCENDING ON ITS OWN: starts holds every s', ends1 every
 * e' + 1 (so it stays unsigned); all values are below 2^31.
 *
 * WINDOWS of a hit, after a scan at guide length l = 1 .. 50, with seed length S, 1 <= S <= l: closed ranges of arena
 * positions in the forward text; pos is the match index i ('+' row, .GG at i) or j ('-' row, CC. at j):
 *               '+' row               '-' row
 *   site        [i - l, i + 2]        [j, j + 2 + l]          guide + PAM
 *   guide       [i - l, i - 1]        [j + 3, j + 2 + l]
 *   seed        [i - S, i - 1]        [j + 3, j + 2 + S]      the PAM-proximal S letters of the guide
 *   pam         [i + 1, i + 2]        [j, j + 1]              the two fixed letters
 * A variant [s, e] TOUCHES a window [a, b] when s <= b and e >= a; an insertion touches it exactly when both letters
 * around its junction lie inside (an insertion between guide and PAM counts for `site` only).  The count of a window is
 * #(starts <= b) - #(ends1 <= a), exact because e >= s - 1.  Every row has a value, the unscored rows and the '-' rows
 * whose window runs past the contig's end included: the void between texts carries no variant.  A substitution at the
 * PAM's N counts in `site` only.
 * One uint32 per row: site | guide << 8 | seed << 16 | pam << 24, each SATURATING at 255. */
/* Host side (no GPU needed): the VCF reader.  Text VCF bytes in any number of chunks (a .gz is unpacked by the caller).
 *   lines     end with LF or CRLF; the last one may lack its line end; empty lines are skipped
 *   # lines   are skipped, except that #CHROM names the samples (columns 10 ...)
 *   columns   tab-separated, at least CHROM POS ID REF ALT; POS a plain digit string >= 1 (at most 15 digits); REF and
 *             every ALT letters of ACGTNacgtn
 *   ALT       comma-separated; `.`, `*`, a symbolic <...> and a breakend (holds [ or ]) are skipped and counted
 *   pass_only the record is kept only if FILTER (column 7) is PASS or `.`
 *   samples   (n_samples > 0; an unknown name is an error, as is a data line before any #CHROM line): ALT allele k is kept
 *             only when the GT of at least one named sample holds k -- GT is found through FORMAT (column 9), its alleles
 *             are split at / and |, `.` is ignored, an index beyond the ALT list is malformed.  Without samples every ALT
 *             allele is kept: a sites-only VCF works.
 * A malformed line is CRP_ERR_INVALID with a crp_variants_error text that names the line number; the handle then refuses
 * further bytes.  Allele-frequency filters and symbolic structural variants (END=) are not read. */
typedef struct crp_variants crp_variants;
int crp_variants_create(const char *const *samples, uint64_t n_samples, int pass_only, crp_variants **out);
int crp_variants_add_bytes(crp_variants *variants, const uint8_t *bytes, uint64_t n);
int crp_variants_finish(crp_variants *variants);
int crp_variants_destroy(crp_variants *variants);
/* The text of the handle's error ("" without one); valid until the handle's next call. */
const char *crp_variants_error(const crp_variants *variants);
/* out[0] lines read, [1] records (data lines), [2] records dropped by pass_only, [3] ALT alleles kept, [4] ALT alleles
 * skipped (`.`, `*`, symbolic, breakend), [5] ALT alleles no named sample carries, [6] ALT alleles equal to REF after
 * stripping, [7] CHROMs with at least one kept allele.  n: how many of these to write (<= 8). */
int crp_variants_stats(const crp_variants *variants, uint64_t *out, int n);
/* CHROM k (order of first appearance among the kept alleles): its name.  The pointer stays valid until
 * crp_variants_destroy.  After crp_variants_finish. */
int crp_variants_chrom(const crp_variants *variants, uint64_t k, const uint8_t **name, uint64_t *name_len);
/* The track of one arena for crp_variant_set_track, after crp_variants_finish (ARENA LAYOUT above).  Capacity protocol
 * of crp_annotation_track: CRP_ERR_CAPACITY with the needed size in *n_out when cap is too small (cap 0: sizing call). */
int crp_variants_track(const crp_variants *variants, const uint64_t *entries, uint64_t n_entries, int dec, uint32_t *starts,
                       uint32_t *ends1, uint64_t cap, uint64_t *n_out);
/* Device side.  The arena keeps a copy of the track in HBM (8 B per variant) with one bucket index per array: entry b is
 * the number of values below b << 11 (the annotation track's scheme), built on the GPU.  n = 0 is a valid, empty track.
 * CRP_ERR_INVALID: an array that is not ascending or holds a value >= 2^31; CRP_ERR_STATE: the arena is not sealed. */
int crp_variant_set_track(crp_arena *arena, const uint32_t *starts, const uint32_t *ends1, uint64_t n);
/* After crp_scan_score on `arena` and crp_variant_set_track: the packed counts of every kept hit, table order.  The
 * column stays in HBM until the arena's next scan (crp_select_set_variant_limits reads it there) and is copied to plus /
 * minus (n_plus / n_minus values; either may be NULL).  One kernel lane per four rows, one launch for both tables; five
 * ranks per row, each two bucket entries and a binary search inside the bucket.  With a crp_last_error text:
 * CRP_ERR_STATE without tables or without a track, CRP_ERR_INVALID for tables scanned at guide length 0 and for a
 * seed_len outside 1 .. l. */
int crp_variant_counts(crp_arena *arena, int seed_len, uint32_t *plus, uint32_t *minus);
/* The last crp_variant_counts of the arena (CRP_ERR_STATE without a column for the current tables): out[0] ms of its
 * kernel (HIP events), out[1] rows, out[2] the guide length, out[3] the seed length, out[4] the track's variants.
 * n: how many of these to write (<= 5). */
int crp_variant_counts_stats(const crp_arena *arena, double *out, int n);
/* Variant limits of a selection (the column of crp_variant_counts): with limits set a row PASSES only if also
 * site <= max_site, guide <= max_guide, seed <= max_seed and pam <= max_pam (the saturated bytes: a limit of 255 or more
 * holds for every row).  Every kernel that evaluates the selection's predicate -- crp_select_run, crp_select_run_pairs,
 * the coding / edit / splice / family evaluations and crp_select_family_step -- then reads 4 more bytes per row
 * (crp_select_stats counts them) and the run returns CRP_ERR_STATE when the arena holds no variant column for its current
 * tables.  NULL clears the limits. */
typedef struct crp_select_variant_limits {
    uint32_t max_site, max_guide, max_seed, max_pam;
} crp_select_variant_limits;
int crp_select_set_variant_limits(crp_select *select, const crp_select_variant_limits *limits);

/* ---- restriction sites: cloning-safe guides and cut-site assays (opt-in) ------------------ */
/* Two questions per kept hit about the recognition sequences of a set of restriction enzymes: does one lie inside the
 * guide (the Golden Gate enzyme of the vector would cut the spacer), and does one span the Cas9 cut while being the only
 * one of its enzyme in the amplicon around it (an indel destroys it: a PCR / restriction-enzyme assay reads the edit).
 *
 * ENZYME SET.  E enzymes, 1 <= E <= 32; enzyme e is bit e of every mask.  An enzyme is a recognition motif M of m
 * letters, 4 <= m <= 16, over the 15 IUPAC letters ACGTRYSWKMBDHVN (case ignored, U read as T); a motif letter stands
 * for a set of bases (R = AG, Y = CT, S = CG, W = AT, K = GT, M = AC, B = CGT, D = AGT, H = ACT, V = ACG, N = ACGT).
 * rc(M) reverses the motif and complements each set (A <-> T, C <-> G).
 *
 * OCCURRENCE.  Enzyme e occurs at arena position q when every letter of s[q : q + m] is a base and lies in the set of
 * the motif letter at its place, for M or for rc(M).  A base is a letter whose `ac` bit is set, with code (hi, lo); the
 * `up` plane is not read (soft-masked text matches like upper case) and a genome U is A as packed.  A non-base matches
 * nothing, not even a motif N: N, IUPAC letters, decoration, void, a position below 0 and a position in a plane word at
 * or beyond the arena's word count.  A palindromic motif occurring at q is ONE occurrence.  Occurrences cannot contain
 * void, so a footprint [q, q + m) always lies inside one text.
 *
 * PER ROW of the hit tables after a scan at guide length l, 1 <= l <= 50, with amplicon half-width A, m_max <= A <=
 * 100 000 (m_max: the set's longest motif); pos is the match index i ('+' row) or j ('-' row):
 *   cut boundary c      i - 3 ('+'), j + 6 ('-'): letters c - 1 and c lie around the cut (section 18's, not the CSV's cutsite)
 *   guide window        [g0, g0 + l), g0 = i - l ('+'), j + 3 ('-') (section 17's: the protospacer without the PAM)
 *   text [t0, t1)       the text of crp_sites_set_enzymes that contains c; where none does the amplicon is empty
 *   in_guide bit e      an occurrence with g0 <= q and q + m <= g0 + l exists (never when m > l)
 *   span_e              occurrences with c - m + 1 <= q <= c - 1: both letters around the cut belong to the site
 *   amp_e               occurrences with max(c - A, t0) <= q and q + m <= min(c + A, t1)
 *   assay bit e         span_e >= 1 and amp_e == 1: the one site of the amplicon is the one across the cut (two
 *                       overlapping sites across the cut give amp_e = 2 and no bit)
 * One uint64 per row: in_guide | assay << 32.  Every row has a value, the unscored rows and the '-' rows whose windows run
 * past the text included; nothing saturates.
 *
 * crp_sites_set_enzymes: the arena (sealed) builds, on the GPU, one occurrence plane per enzyme over its plane words (bit p
 * of word w: an occurrence at 64 w + p) and a rank index (uint32 per word: the occurrences below 64 w), and keeps the
 * texts' bounds: 12 B per plane word and enzyme of device memory, held until the arena is reset or destroyed -- re-scans
 * keep them.  motifs[e] holds lens[e] letters (no terminator needed); text_starts / text_ends: n_texts half-open ranges
 * of arena positions, ascending and disjoint.  CRP_ERR_INVALID with a crp_last_error text: E outside 1 .. 32, m outside
 * 4 .. 16, a letter outside the alphabet, bounds that do not ascend or leave the arena; CRP_ERR_STATE: not sealed;
 * CRP_ERR_NOMEM with a text that names the size when the planes do not fit.  A new set drops the column of the old one. */
int crp_sites_set_enzymes(crp_arena *arena, uint64_t n, const char *const *motifs, const uint32_t *lens, const uint32_t *text_starts,
                          const uint32_t *text_ends, uint64_t n_texts);
/* After crp_scan_score and crp_sites_set_enzymes: the value of every kept hit, table order.  The column stays in HBM until
 * the arena's next scan or enzyme set (crp_select_set_site_limits reads it there) and is copied to plus / minus (n_plus /
 * n_minus values; either may be NULL).  One kernel lane per row, one launch for both tables.  With a crp_last_error text:
 * CRP_ERR_STATE without tables or without an enzyme set, CRP_ERR_INVALID for tables scanned at a guide length outside
 * 1 .. 50 and for a flank outside m_max .. 100 000.  Empty tables are fine. */
int crp_site_columns(crp_arena *arena, int flank, uint64_t *plus, uint64_t *minus);
/* The arena's enzyme set and its last crp_site_columns (CRP_ERR_STATE without a set): out[0] ms of the plane build,
 * out[1] ms of the rank build, out[2] ms of the column kernel (HIP events), out[3] rows, out[4] E, out[5] A, out[6] bytes of
 * device memory the planes and ranks hold; [2], [3] and [5] are 0 without a column for the current tables.  n: how many of
 * these to write (<= 7). */
int crp_site_stats(const crp_arena *arena, double *out, int n);
/* Site limits of a selection (the column of crp_site_columns): with a mask set a row PASSES only if also no enzyme of
 * forbid_mask lies inside its guide and -- need_mask != 0 -- it has an assay with at least one enzyme of need_mask.  Every
 * kernel that evaluates the selection's predicate then reads 8 more bytes per row (crp_select_stats counts them) and the
 * run returns CRP_ERR_STATE when the arena holds no site column for its current tables.  0 / 0 clears the limits. */
int crp_select_set_site_limits(crp_select *select, uint32_t forbid_mask, uint32_t need_mask);

/* ---- options -------------------------------------------------------------- */
/* CRP_OPT_TWO_PASS (value 0/1, default 0): with 0 crp_scan_score is ONE kernel launch; the
 * table offsets come from a chained scan across workgroups inside it (decoupled look-back
 * over per-tile descriptors; every wait is bounded in wall time).  With 1 it runs the count /
 * tile-scan / emit+score launch sequence (one more pass over the packed planes).  Results
 * are identical; the single launch is ~20 % faster per scan on MI355X.
 * A scan in which a look-back ran out of its allowance is repeated with the three-launch
 * sequence (see CRP_OPT_CHAIN_TIMEOUT_US); the setting itself is not changed by that. */
#define CRP_OPT_TWO_PASS 1
/* CRP_OPT_CHAIN_TIMEOUT_US (default 20000): how long a workgroup of the single-launch scan waits for
 * a predecessor's counts before it gives up (wall time, read from the GPU's 100 MHz real-time
 * counter).  A scan in which a wait ran out is repeated with the three-launch sequence; the next scan
 * tries the single launch again.  Only after three such scans in a row does the context stay with
 * three launches (crp_query reports both). */
#define CRP_OPT_CHAIN_TIMEOUT_US 2
/* CRP_OPT_TILE_GEOMETRY (default 0): the tile shape crp_arena_seal gives the arenas sealed AFTER the call.  The scan works
 * tile by tile, one workgroup per tile; results do not depend on the shape, time does:
 *   0  by the arena's size against the GPU: SMALL when the arena holds fewer than 1.5 LARGE tiles per CU (E. coli-like:
 *      one tile's life is the whole kernel), LARGE otherwise
 *   1  LARGE   512 threads on 1 024 words (65 536 positions), two words per lane: the throughput shape
 *   2  SMALL   512 threads on 512 words, one word per lane: half the rows per lane, half the tile's life */
#define CRP_OPT_TILE_GEOMETRY 3
/* CRP_OPT_PREFETCH_TILES (default -1; also read from the environment variable of the same name when the context is
 * created): in the single-launch scan, a tile that is done with its rows asks for the planes of the tile that many tiles
 * after it, so that the tile finds them in the L2.  -1: the distance crp_arena_seal chose for the
 * arena from the GPU's size; 0: no prefetch; any other value is used as given (a multiple of 8 keeps requester and
 * target on one XCD).  Results do not depend on it.  Applies to the scans launched after the call. */
#define CRP_OPT_PREFETCH_TILES 4
int crp_configure(crp_ctx *ctx, int option, int64_t value);

/* Read-only state, for logs and bench output. */
#define CRP_Q_CHAIN_TIMEOUTS 1   /* single-launch scans that had to be repeated with three launches */
#define CRP_Q_TWO_PASS_ACTIVE 2  /* 1 when scans currently run as three launches (configured or latched) */
#define CRP_Q_COMM_WORLD 3       /* ranks of the RCCL communicator (0: none) */
#define CRP_Q_COMM_RANK 4
#define CRP_Q_HBM_FREE 5         /* bytes of device memory free right now, as hipMemGetInfo sees the whole device (all processes) */
#define CRP_Q_HBM_TOTAL 6
#define CRP_Q_GATHER_BYTES 7     /* last crp_gather_hits: bytes this rank sent to the root (a peer) or received from all peers (the root) */
int crp_query(const crp_ctx *ctx, int what, int64_t *value);
/* Identifies the build: a hash of the library's sources taken by the Makefile ("unknown" otherwise).
 * profiles/traffic.json carries the id of the build it was measured on; bench.py refuses another. */
const char *crp_build_id(void);

/* ---- measurement --------------------------------------------------------- */
/* on = 1: the emit+score kernel of every crp_scan_score is bracketed by HIP events
 * on the stream it is launched on; on = 2: all three kernels; 0: off. */
int crp_profile_enable(crp_ctx *ctx, int on);
/* Sum of durations (ms) and launch count per kernel since the last reset:
 * index 0 = count pass, 1 = tile-offset scan (both only with CRP_OPT_TWO_PASS = 1),
 * 2 = emit+score pass (the whole scan with CRP_OPT_TWO_PASS = 0). */
int crp_profile_read(crp_ctx *ctx, double ms[3], uint64_t launches[3], int reset);
/* The same for any kernel kind (ms and launches since the last reset of that kind). */
#define CRP_K_COUNT 0
#define CRP_K_TILE_SCAN 1
#define CRP_K_EMIT 2
#define CRP_K_OT_SEED 3      /* off-target: seeds of the kept hits + site histogram */
#define CRP_K_OT_BALL 4      /* off-target: the three Hamming-ball passes together */
#define CRP_K_OT_LOOKUP 5    /* off-target: per-hit counts */
#define CRP_K_GATHER 6       /* RCCL gatherv of the hit tables (count all-gather + grouped send/recv) */
#define CRP_K_OT_REDUCE 7    /* RCCL all-reduce of the site histogram */
#define CRP_K_ANNOTATE 8     /* annotation join: the look-up kernel of one crp_annotate_lookup (both tables, one launch) */
#define CRP_K_PROPERTIES 9   /* guide properties: the kernel of one crp_guide_properties (both tables, one launch) */
#define CRP_K_KINDS 10
int crp_profile_read_kind(crp_ctx *ctx, int kind, double *ms, uint64_t *launches, int reset);
/* Blocks until everything queued on the library's stream has finished. */
int crp_synchronize(crp_ctx *ctx);
/* Number of rows of the last crp_scan_score that carry a real score (not -1), counted on the GPU:
 * the unit of the "gRNAs scored" metric. */
int crp_count_scored(crp_arena *arena, uint64_t *n_scored);

#ifdef __cplusplus
}
#endif
#endif /* CROPSR_HIP_H */
