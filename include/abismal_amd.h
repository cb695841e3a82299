/* abismal_amd — C ABI of the MI355X-native mapping path.
 *
 * The reference (smithlabcode/abismal v3.3.0) has no FFI; its seam for this
 * path is the body of the per-read loops in src/abismal.cpp — everything
 * between ReadLoader::load_reads (:1545) and format_se / select_output
 * (:1577, :2000).  Each entry point below names the reference code it
 * replaces.  All functions return 0 on success, <0 on error (text via
 * abm_last_error()); no ownership is transferred; plain pointers and sizes
 * only.
 */
#ifndef ABISMAL_AMD_H
#define ABISMAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct abm_index abm_index; /* host copy of an AbismalIndex file */
typedef struct abm_ctx abm_ctx;     /* one GPU: index in HBM + workspaces */

/* se_element, src/abismal.cpp:224-297.  pos is the absolute position in the
 * padded concatenated genome; pos == 0 means "no hit" (flags/diffs are then
 * unspecified).  flags: 0x10 reverse strand, 0x100 ambiguous, 0x1000 A-rich. */
typedef struct { int16_t diffs; uint16_t flags; uint32_t pos; } abm_hit;

/* pe_element, src/abismal.cpp:547-619 (aln_score + both ends) */
typedef struct { int16_t aln_score; int16_t reserved; abm_hit r1, r2; } abm_pair;

/* the tunables the path reads: src/abismal.cpp:2329-2337, :2448-2452 */
typedef struct {
  uint32_t max_candidates; /* 0 = value stored in the index (-c) */
  double valid_frac;       /* -m, default 0.1 */
  uint32_t min_frag;       /* -l, default 32 (PE) */
  uint32_t max_frag;       /* -L, default 3000 (PE) */
  int32_t allow_ambig;     /* -a: only steers the PE single-end fallback */
} abm_params;

/* conversion modes = which per-read body runs */
enum { ABM_SE_T_RICH = 0, ABM_SE_A_RICH = 1, ABM_SE_RANDOM = 2 }; /* :1552-1581, -A/-P, :1645-1685 */
enum { ABM_PE_NORMAL = 0, ABM_PE_PBAT = 1, ABM_PE_RANDOM = 2 };   /* :1950-2002, -P, :2094-2158 */

const char *abm_last_error(void);
int abm_device_count(void); /* HIP devices visible to the process (0 = none: every abm_ctx_create will fail) */
/* NUMA node of the host memory nearest to `device` (from its PCI address; -1 = unknown): where a host driver places
 * the threads and buffers that feed that GPU (no reference counterpart: its worker threads are not placed). */
int abm_device_numa_node(int device);
/* Page-locked host memory, usable from every device (hipHostMalloc, portable): batches whose seq_blob / seq_off lie
 * in it are uploaded by the DMA engines at the link's rate instead of through the runtime's staging buffers (the
 * reference has no counterpart: its batches never leave the host). */
int abm_host_alloc(size_t bytes, void **out);
void abm_host_free(void *p);
void abm_default_params(abm_params *p);

/* AbismalIndex::read, src/AbismalIndex.cpp:1082-1146 (+ seed::read :988-1024,
 * ChromLookup::read :1225-1258).  Rejects files whose identifier or seed
 * constants (25 / 20 / 256) differ, with the reference's messages. */
int abm_index_open(const char *path, abm_index **out);
void abm_index_close(abm_index *ix);
uint32_t abm_index_max_candidates(const abm_index *ix);
uint32_t abm_index_n_chroms(const abm_index *ix);              /* incl. pad_start/pad_end */
const char *abm_index_chrom_name(const abm_index *ix, uint32_t i);
const uint32_t *abm_index_chrom_starts(const abm_index *ix);    /* n_chroms+1 entries */
uint64_t abm_index_bytes(const abm_index *ix);                  /* bytes resident in HBM after upload */

/* `abismal idx <genome.fa> <out.idx>` (src/abismalidx.cpp:35-115 ->
 * AbismalIndex::create_index + write, src/AbismalIndex.cpp:281-331, :1037-1072).
 * Host-side, multi-threaded; the file is byte-identical to the reference's. */
int abm_index_build(const char *fasta_path, const char *out_path, uint32_t n_threads);
/* `abismal idx -A <targets> ...` (AbismalIndex::create_index(targets, genome), src/AbismalIndex.cpp:206-279):
 * only the regions listed in targets_path ("chrom start end" per line) are indexed; NULL or "" = whole genome. */
int abm_index_build_targets(const char *fasta_path, const char *targets_path, const char *out_path, uint32_t n_threads);
/* The same with the seed window chosen: 20 (default) or 12, the reference's --enable-short build for short reads
 * (configure.ac:70-73, src/AbismalIndex.hpp:73-77: shortest mappable read 36 instead of 44 bases).  The window is
 * stored in the index file; abm_index_open takes either and the mapping entry points follow it. */
int abm_index_build_opts(const char *fasta_path, const char *targets_path, uint32_t window, const char *out_path,
                         uint32_t n_threads);
uint32_t abm_index_window(const abm_index *ix);

/* Seed-extension tables (no reference counterpart; results are unaffected).  The first context on a device also
 * derives, in HBM, three tables that answer the first steps of the bucket-narrowing loops of find_candidates /
 * find_candidates_three (src/abismal.cpp:1163-1259) with one load per seed offset: one entry per key of the hashed
 * letters plus letters2 more (2-letter table, at most 7) / letters3 more (3-letter tables, at most 4).  By default
 * the letters are chosen from the genome's length (none below 33 Mbp; 7 and 4 = 90 GB at hg38 scale, fewer if that
 * exceeds half of the free device memory); this call fixes them (0, 0 = no tables) and must precede the first
 * abm_ctx_create on the index.  The tables are built for the index's max_candidates (or the value given to
 * abm_index_set_max_candidates before the context was created); a call with another value runs without them --
 * nothing is ever rebuilt inside a mapping call.  abm_ctx_rebuild_seed_extension rebuilds them explicitly. */
int abm_index_set_seed_extension(abm_index *ix, int letters2, int letters3);
/* The automatic choice (letters from the index's size) capped at these (0, 0 = no tables).  At hg38 scale 7 + 4 letters are
 * 90 GB, 6 + 3 are 36 GB, 4 + 2 are 10 GB; since the kernels narrow every range beyond max_candidates directly the tables
 * are worth 3.7 / 3.1 / 2 % of the single-end kernel's time and nothing to the pair kernels
 * (profiles/r05_exp_e2e_and_tables.log) -- so a host that maps pairs caps at 0 and 0.  Contexts created afterwards. */
int abm_index_set_seed_extension_cap(abm_index *ix, int letters2, int letters3);
/* Window records (no reference counterpart; results are unaffected).  check_hits (src/abismal.cpp:1124-1150) compares
 * the read with the genome at every entry of a checked bucket: one random gather per candidate, and at hg38 scale 2,800
 * of them per 100-base read -- the line requests that bound the mapping kernels.  With 288 GB of HBM the index can carry
 * its candidates' windows itself: for every index entry the stretch of the genome (as bit planes, 2 bits per base) that
 * a window of a read of up to max_read_len bases can lie in, entries in index order, so that a bucket's windows are
 * consecutive 48-byte records (reads up to 108 bases; 64 bytes up to 140, 80 up to 172) instead of one 128-byte line
 * each.  8.4 GB at hg38 scale for 100-base reads.  Reads longer than the records serve are filtered from the bit planes
 * as before.  0 = none (the default); must precede the first abm_ctx_create on the index.  abm_ctx_window_records: the
 * longest read the context's records serve (0: none were built -- no planes, or not enough free device memory). */
int abm_index_set_window_records(abm_index *ix, int max_read_len);
uint32_t abm_ctx_window_records(const abm_ctx *ctx);
/* Bit planes for genomes with IUPAC letters (no reference counterpart; results are unaffected).  One ambiguity letter
 * (R, Y, M, K, S, W, B, D, H, V: a genome nibble with two or more bits) otherwise takes the whole device off the bit
 * planes -- and with them off the window records, direct narrowing and device-written records: every launch then is the
 * nibble build.  on != 0: the genome keeps its planes, and such letters are marked as blank nibbles (N) are -- in the
 * planes' map of 4096-base chunks and in the window records' flags -- so that only the windows and probes within reach
 * of one go back to the nibble array.  No seed-extension tables for such genomes either way.  On a genome without such
 * letters the option changes nothing.  Default 0; must precede the first abm_ctx_create on the index.
 * abm_ctx_plane_chunks: the chunks of the context's genome and how many of them are marked (blanks and IUPAC letters
 * together): the share of the genome that goes the slow way.  0 and 0 when the context has no planes. */
int abm_index_set_iupac_planes(abm_index *ix, int on);
int abm_ctx_plane_chunks(const abm_ctx *ctx, uint64_t *chunks, uint64_t *flagged);
/* the max_candidates (-c, src/abismal.cpp:2329) the calls on this index will pass, when it is not the value stored
 * in the index file: the tables of contexts created afterwards are built for it (0 = the file's value) */
int abm_index_set_max_candidates(abm_index *ix, uint32_t max_candidates);
/* The mapping kernels narrow a seed's big ranges -- seeds inside high-copy repeats -- directly: find_candidates /
 * find_candidates_three (src/abismal.cpp:1163-1259) extend such a seed letter by letter, a bisection of the range per
 * letter; the same final range comes out of one bisection with whole-string comparisons plus ~30 probes (buckets are
 * sorted by those letters, src/AbismalIndex.cpp:857-978).  Results are unaffected.  min_entries: the smallest range
 * taken that way (default 64: every range beyond the default max_candidates; 0 = never); takes effect with the next call on any context of the index.  (Paired-end
 * calls since round 3, single-end calls since round 5.) */
int abm_index_set_direct_narrowing(abm_index *ix, uint32_t min_entries);
/* Rebuilds the tables of the context's device for another max_candidates (0 = the index file's).  Waits for the device,
 * frees and allocates the tables' memory and runs for seconds at hg38 scale: a set-up call, allowed only while the
 * context is the only one on its device. */
int abm_ctx_rebuild_seed_extension(abm_ctx *ctx, uint32_t max_candidates);
/* what the context's device holds: letters per table (0 = no tables) and their bytes */
int abm_ctx_seed_extension(const abm_ctx *ctx, uint32_t *letters2, uint32_t *letters3, uint64_t *bytes);

/* A context = one host thread's workspaces and stream on `device` (hipSetDevice
 * ordinal).  The first context on a device replicates the index into its HBM;
 * later ones share that replica (freed with the last of them).  Calls on one
 * context are serialised; use one context per mapper thread so that a batch's
 * transfers overlap another batch's kernels.  Destroy every context before
 * abm_index_close. */
int abm_ctx_create(const abm_index *ix, int device, abm_ctx **out);
/* Optional set-up: sizes the context's workspaces for host-buffer batches of up to n reads (pairs, if paired != 0)
 * of up to max_len bases and runs a few dummy reads through the kernels, so that the first real batch pays neither
 * allocations nor code loading (the reference's counterpart: the per-thread scratch built before the batch loop,
 * src/abismal.cpp:1535-1539, :1919-1929). */
int abm_ctx_reserve(abm_ctx *ctx, uint64_t n, uint32_t max_len, int paired);
void abm_ctx_destroy(abm_ctx *ctx);
/* Device memory: free and total bytes of `device` right now (hipMemGetInfo), and what one more context's workspaces for
 * paired-end batches of n pairs of up to max_len bases will take once reserved -- for a host that has to decide how many
 * mapper contexts fit beside the index (no reference counterpart: the reference's per-thread scratch is host memory). */
int abm_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
int abm_ctx_pe_footprint(abm_ctx *ctx, uint64_t n, uint32_t max_len, uint64_t *bytes);

/* Single-end batch, host buffers.  Replaces the loop body of
 * map_single_ended / map_single_ended_rand (src/abismal.cpp:1552-1576,
 * :1645-1680): reads are the strings ReadLoader would hand over (already
 * N-trimmed; empty = skipped), concatenated in seq_blob with n+1 offsets.
 * A trimmed read may be shorter than the reader's minimum of key weight +
 * window - 1 letters (it began with IUPAC letters, which the reader counts and
 * then trims, :187-195); the reference maps it all the same, and so does this
 * library down to 35 bases (29 with a short-read index): below that a read
 * is left unmapped like an empty one.
 * out_res[i] equals bests[i] and the CIGAR equals r[i].cig just before
 * format_se; CIGAR ops are BAM-encoded (len<<4|op) in out_cig_blob with n+1
 * offsets in out_cig_off (reads without a hit get an empty CIGAR).
 * cig_capacity is out_cig_blob's size in ops: a few ops per read are typical,
 * at most read length + 2; ABM_ERR_CAPACITY (-2) is returned if it does not
 * suffice, and the call can be repeated with a larger buffer.
 * The caller's buffers may be ordinary (pageable) memory: the kernel writes its
 * results into pinned staging buffers of the context (grow-only, see
 * abm_ctx_reserve) and the call copies them out on a few host threads, so
 * nothing has to cross the bus after the kernel while another context's batch
 * occupies the device. */
#define ABM_ERR_CAPACITY (-2)
int abm_map_se_batch(abm_ctx *ctx, int mode, const abm_params *params, uint64_t n,
                     const char *seq_blob, const uint64_t *seq_off, abm_hit *out_res,
                     uint32_t *out_cig_blob, uint64_t cig_capacity, uint64_t *out_cig_off);

/* The same batch with its results handed over SLICE BY SLICE while the kernel is still running -- for a caller that
 * formats and writes output as it arrives (the reference's counterpart: its output loop runs per batch after the
 * mapping loop, src/abismal.cpp:1578-1598; a GPU batch is millions of reads, and waiting for all of it leaves the
 * host idle for the length of a kernel and then the device idle for the length of the formatting).
 * slice_first: n_slices + 1 read indices, non-decreasing, the last one n; reads before slice_first[0] belong to no
 * slice (a batch's lead-in, mapped for its effect on later reads only).  The kernel works through the batch's few
 * heaviest reads first and then slice after slice; when a slice's last read is done, `done(user, slice)` is called
 * on the calling thread, and INSIDE that call abm_ctx_slice_results copies the slice's reads [lo, hi) out of the
 * context's pinned buffers: hits, and CIGARs as a compact blob with hi - lo + 1 offsets relative to the range
 * (ABM_ERR_CAPACITY if cig_capacity ops do not suffice; out_cig_off[hi - lo] then holds the number needed).  After
 * `done` returns the slice's results may be overwritten.  Every slice is handed over exactly once before the call
 * returns; slices of a batch with reads of more than 1024 bases all arrive at the end. */
typedef void (*abm_slice_done_fn)(void *user, uint32_t slice);
int abm_map_se_batch_sliced(abm_ctx *ctx, int mode, const abm_params *params, uint64_t n,
                            const char *seq_blob, const uint64_t *seq_off, uint32_t n_slices,
                            const uint64_t *slice_first, abm_slice_done_fn done, void *user);
int abm_ctx_slice_results(abm_ctx *ctx, uint64_t lo, uint64_t hi, abm_hit *out_res,
                          uint32_t *out_cig_blob, uint64_t cig_capacity, uint64_t *out_cig_off);

/* SAM text from the device (round 5; the reference's counterpart: format_se, src/abismal.cpp:481-545, run per read on the
 * host after the mapping loop).  When enabled, the single-end kernel of abm_map_se_batch_sliced also writes, for every
 * read, its SAM line after QNAME -- "\tFLAG\tRNAME\tPOS\t255\tCIGAR\t*\t0\t0\tSEQ\t*\tNM:i:n\tCV:A:c\n", byte for byte what
 * format_se + htslib's SAM writer print: the wave that mapped the read holds hit, CIGAR and conversion type, the reads'
 * text is on the device, and the chromosome table rides with the index -- so that the host's formatting of a record is
 * two copies (name, tail).  allow_ambig: the run's -a (ambiguous hits are written, flag 0x100).
 * Inside the slice callback, abm_ctx_slice_sam_tails hands out the context's pinned buffers for reads [lo, hi): tails at
 * *tails + k * *stride, lens[k] bytes each -- 0: the read has no record (unmapped, ambiguous and not allowed, or a hit
 * that runs across its chromosome's end), 0xFFFFFFFF: not written by the device (a CIGAR beyond its 4-op slot, a read of
 * more than 1024 bases, a line beyond the slot): format that one from abm_ctx_slice_results as before.  *tails is NULL
 * when the launch wrote none.  Valid until the callback returns. */
int abm_ctx_set_sam_tails(abm_ctx *ctx, int enable, int allow_ambig);
int abm_ctx_slice_sam_tails(abm_ctx *ctx, uint64_t lo, uint64_t hi, const char **tails, uint32_t *stride, const uint32_t **lens);
/* The same for pairs: with tails enabled, abm_map_pe_batch's kernels also write, for every pair, the records that
 * select_output prints (src/abismal.cpp:1073-1088), minus QNAME -- a proper pair's two records (format_pe, :648-773:
 * flags 0x1|0x2|0x40 / 0x80, 0x10 / 0x20 by strand, 0x100 with allow_ambig; RNEXT "=", PNEXT the mate's POS, TLEN
 * +-isize; each end its own NM and CV), or else up to two single-end records (format_se: RNEXT "*", 0, 0).  After the
 * call, abm_ctx_pe_sam_tails hands out the context's pinned buffers for pairs [lo, hi) of that batch: the tail of end e
 * of pair lo + k at *tails + (2k + e) * *stride, lens[2k + e] bytes long (0: that end has no record), and kinds[k]:
 *   0     the pair's two records;
 *   1     single-end fallback records (also a pair whose ends cannot both be located on one chromosome: unmapped as a
 *         pair);
 *   0xFF  nothing written: format this pair from the batch's results as before (an end of more than 1024 bases, a CIGAR
 *         of more than 50 ops, a line beyond its slot).
 * The stride is computed per batch from its longest end.  *tails (and lens, kinds) is NULL when the batch wrote none:
 * text needs a genome without IUPAC letters (the filter on bit planes), no phase stamps, and a slot that fits the LDS a
 * line is built in (the single-end launches apply the same guard).  Valid until the context's next mapping call. */
int abm_ctx_pe_sam_tails(abm_ctx *ctx, uint64_t lo, uint64_t hi, const char **tails, uint32_t *stride,
                         const uint32_t **lens, const uint8_t **kinds);
/* BAM pieces in the place of SAM text.  With ABM_RECORDS_BAM the same kernels write, into the same slots and under the
 * same conditions, each record as a BAM piece -- the record `abismal-amd map -B` writes, without the read's name, which
 * only the host has.  lens and kinds keep their meanings (0: no record; 0xFFFFFFFF / kind 0xFF: the host formats it --
 * besides the cases above, a CIGAR of more ops than the slot was sized for: 4 single-end, 8 per end of a pair).
 * A piece of `len` bytes:
 *   [0, 36)    block_size and the 32 fixed bytes of a BAM alignment record (SAM specification 4.2), little-endian, with
 *              l_read_name = 0 and block_size counting the record WITHOUT its name: refID and pos (0-based) on the BAM
 *              header's chromosome list, MAPQ 255, bin = reg2bin(pos, pos + max(reference length, 1)), n_cigar_op,
 *              FLAG, l_seq, then next refID / next pos / TLEN -- the mate's for a proper pair, else -1, -1, 0;
 *   [36, len)  the CIGAR ops (length << 4 | op), SEQ two bases a byte (high nibble first, codes of "=ACMGRSVTWYHKDBN",
 *              the low nibble of the last byte 0 when l_seq is odd; a reverse-strand hit shows the reverse complement),
 *              l_seq bytes 0xFF (no qualities), "NM" with the smallest of the types C, S, c, s that holds the value, and
 *              "CV" "A" with the conversion letter.
 * The host makes a record of a piece in four steps: copy the 36 bytes; add strlen(name) + 1 to block_size and store
 * (uint8_t)(strlen(name) + 1) as l_read_name (byte 12); append the name and a NUL; append bytes [36, len).
 * SAM is the default.  The format takes effect with the context's next mapping call (call it before abm_ctx_reserve, which
 * sizes the slots for the format that is set) and has no effect while abm_ctx_set_sam_tails is off.  A null context or
 * an unknown value is an error (< 0, text in abm_last_error()). */
enum { ABM_RECORDS_SAM = 0, ABM_RECORDS_BAM = 1 };
int abm_ctx_set_record_format(abm_ctx *ctx, int format);

/* Same computation with every buffer already resident in HBM (d_* are device
 * pointers), enqueued on `stream` (a hipStream_t; NULL = default stream) and
 * not synchronised.  CIGARs land in fixed slots of cig_stride ops per read,
 * their op counts in d_cig_n.  A CIGAR with more ops than cig_stride (its count
 * says so) lies whole in the context's arena instead, beginning at the index its
 * slot's first word holds; abm_ctx_long_cigars() returns the arena of the last
 * call.  ABM_STATUS_CIGAR_OVERFLOW is only set if the arena itself ran out (one op
 * per read by default), in which case such slots hold what fitted: the CIGAR's first
 * cig_stride ops.  d_status (one
 * uint32) is OR-ed with ABM_STATUS_* bits. max_len = longest read in the batch.
 * A context owns ONE set of workspaces: a device call first makes `stream` wait
 * for the context's previous device call (on whatever stream that ran), so calls
 * on one context execute one after the other; use one context per stream to
 * overlap batches.  Growing a workspace frees the old one, which synchronises
 * the device once -- size-stable batches never pay that. */
int abm_map_se_device(abm_ctx *ctx, int mode, const abm_params *params, uint64_t n,
                      const char *d_seq_blob, const uint64_t *d_seq_off, uint32_t max_len,
                      abm_hit *d_res, uint32_t *d_cig, uint32_t cig_stride, uint32_t *d_cig_n,
                      uint32_t *d_status, void *stream);

/* Paired-end batch.  Replaces the loop body of map_paired_ended /
 * map_paired_ended_rand (src/abismal.cpp:1950-1999, :2094-2155): out_pair[i],
 * out_se1[i], out_se2[i] and the two CIGARs equal bests[i], bests_se1[i],
 * bests_se2[i], r1[i].cig, r2[i].cig just before select_output. */
int abm_map_pe_batch(abm_ctx *ctx, int mode, const abm_params *params, uint64_t n,
                     const char *seq_blob1, const uint64_t *seq_off1, const char *seq_blob2,
                     const uint64_t *seq_off2, abm_pair *out_pair, abm_hit *out_se1,
                     abm_hit *out_se2, uint32_t *out_cig_blob1, uint64_t *out_cig_off1,
                     uint32_t *out_cig_blob2, uint64_t *out_cig_off2, uint64_t cig_capacity);

int abm_map_pe_device(abm_ctx *ctx, int mode, const abm_params *params, uint64_t n,
                      const char *d_seq_blob1, const uint64_t *d_seq_off1, const char *d_seq_blob2,
                      const uint64_t *d_seq_off2, uint32_t max_len, abm_pair *d_pair,
                      abm_hit *d_se1, abm_hit *d_se2, uint32_t *d_cig1, uint32_t *d_cig2,
                      uint32_t cig_stride, uint32_t *d_cig_n1, uint32_t *d_cig_n2,
                      uint32_t *d_status, void *stream);

/* How a paired-end batch is launched (no reference counterpart: the reference's per-pair body is one function,
 * src/abismal.cpp:1950-1999).  By default the body is split where its register pressure is: a SEED kernel runs both
 * seed passes of every orientation call's two ends (process_seeds into pe_candidates, :1269-1375, :775-863) and hands the
 * finished candidate lists over in device memory; MATE kernels take them from there (prepare_for_mating, best_pair,
 * best_single, the single-end fallback: :844-852, :1715-1831).  Pairs whose sets outgrow the seed kernel are mapped whole
 * by one wave each with 32768-entry sets, as every heavy pair was before round 5.  Results do not depend on any of this.
 *   split      -1 = default (split), 0 = seeding and mating in ONE kernel per pair (rounds 1-4; same-box comparisons), 1 = split
 *   seed_cap   entries a candidate list may reach inside the seed kernel (0 = default; up to 128 a list stays in LDS,
 *              beyond that it moves to a per-wave staging area in device memory; at most 16384)
 *   hand_entries  list entries the hand-over area holds (0 = default: a multiple of the batch size; a list that finds
 *              no room sends its pair through the whole-pair kernel -- slower, never wrong) */
int abm_ctx_set_pe_split(abm_ctx *ctx, int split, uint32_t seed_cap, uint64_t hand_entries);
/* Measurement hook: pairs by route since the previous call, then reset -- out[0] mated from LDS lists, out[1] mapped
 * whole (sets that outgrew the seed kernel), out[2] mated from lists in device memory -- and out[3] the hand-over entries
 * the context's last batch asked for (waits for the device). */
int abm_ctx_pe_split_stats(abm_ctx *ctx, uint64_t out[4]);
/* HIP-event brackets (abm_ctx_set_timing) the context's last paired-end call recorded, in launch order: split -- seed,
 * mate (LDS lists), mate (lists in device memory), whole pairs = 4; unsplit -- tier 1, tier 2 = 2. */
uint32_t abm_ctx_pe_timed_launches(const abm_ctx *ctx);
/* Test hook: which builds of the mapping kernels the context's last mapping call launched, in launch order (a launch
 * in rounds counts once).  Returns their number and writes the first `cap` of them: each build's id to `ids`, the LDS
 * bytes a wave of that launch took to `lds_bytes` (either may be null).  An id packs the build's fields.  Bit 31 set,
 * single-end: bit 0 timed, 1 coop, 2 rec, 3 bam, 4 is_long, bits 9-12 waves per SIMD.  Bit 31 clear, pairs: bits 0-1
 * phase (0 whole, 1 seed, 2 mate), bit 2 big, 3 is_long, 4 timed, 5 coop, 6 rec, 7 text, 8 bam, bits 9-12 waves per SIMD. */
uint32_t abm_ctx_last_forms(const abm_ctx *ctx, uint32_t *ids, uint32_t *lds_bytes, uint32_t cap);
/* page-locked host memory the context holds for results on their way out (its pinned staging buffers, SAM text
 * included), bytes */
uint64_t abm_ctx_pinned_bytes(const abm_ctx *ctx);

/* the arena of CIGARs longer than their slot left by the context's last device call (waits for it) */
int abm_ctx_long_cigars(abm_ctx *ctx, uint32_t *out_ops, uint64_t capacity, uint64_t *n_ops);

enum {
  ABM_STATUS_CIGAR_OVERFLOW = 1u, /* the arena for CIGARs longer than a slot ran out */
  ABM_STATUS_READ_TOO_LONG = 2u,  /* a read (or an end of a pair) exceeded abm_max_read_length() */
  ABM_STATUS_SET_OVERFLOW = 4u    /* PE candidate set outgrew its workspace */
};
/* Longest read (single-end, or end of a pair) that is mapped: 32766 bases, the reference's own limit (ReadLoader refuses
 * reads of 32767 bases or more, src/abismal.cpp:179-185).  Reads of up to 1024 bases are mapped by a batch's main
 * launch; longer ones -- and pairs with such an end -- by a launch of their own afterwards (traceback tables, and for
 * pairs the read data too, in global memory; the device entry point then waits once for the device, to learn how many
 * there are). */
uint32_t abm_max_read_length(void);
/* Reads (pairs with an end) beyond abm_max_read_length() handed to this context's host entry points so far: they come
 * back without a hit, everything else in their batch is mapped as usual. */
uint64_t abm_ctx_reads_too_long(abm_ctx *ctx);

/* Which form of the genome the Hamming filter of this context's device reads for batches of reads up to 448 bases:
   1 = the bit planes derived at upload (cooperative window loads; every genome without IUPAC ambiguity letters),
   0 = the nibble array, one lane per window (genomes with IUPAC letters).  Results are the same; the rate is not. */
int abm_ctx_filter_on_planes(const abm_ctx *ctx);

/* Measurement hook (no reference counterpart): exact work tallies accumulated by the launches on this context since
 * the previous call, then reset:
 * [0] seed offsets probed, [1] bucket-narrowing search probes (genome letters loaded: a probe that serves both bisections
 * of a 3-letter step counts once), [2] candidates compared, [3] read words compared (the words fetched per candidate
 * window: 6 / 8 / 2 per 64-base block on the bit planes by lane group, 6 / 8 on window records, the read's own on the
 * nibble array), [4] candidate-set updates, [5] alignments scored, [11] candidates served by the position cache (none
 * on window records), [12] single-end reads whose set held one alignable entry.
 * The DIAGNOSTIC builds keep them (abm_ctx_set_phase_stamps).  The production builds keep no seed-pass count -- they
 * cost registers: the single-end kernel returns zeros throughout; the paired-end kernels return zeros in [0]-[3] and
 * [11] and only what costs them nothing: [4] the updates of the single-end sets alone (best_single), [5] alignments.
 * Feeds the algorithmic-bytes model of SURVEY.md section 8(d). */
int abm_ctx_take_work(abm_ctx *ctx, uint64_t out[16]);
/* Diagnostic build of the mapping kernel: adds s_memtime stamps per phase;
 * take_work then also returns summed shader cycles in [6] probe+narrow,
 * [7] candidate gather+Hamming, [8] ordered replay, [9] alignment, [10] total.
 * Never enable it for a run whose time is quoted. */
int abm_ctx_set_phase_stamps(abm_ctx *ctx, int enable);
/* Paired-end runs keep separate tallies per tier: out[0..15] tier 1 (sets of up
 * up to 256 entries), out[16..31] tier 2 (the pairs redone with 32768-entry
 * sets); take_work returns their sum.  In the paired-end tallies [3] is the number of 128-byte lines the checked
 * buckets' index-entry runs span (the fetched windows' words follow from [2] and [11]).  With phase stamps the paired-end kernel
 * fills [6] probe+narrow, [7] gather+Hamming, [8] replay, [9] single-end
 * fallback, [10] total, [12] sort+unique, [13] pairable-entry alignments,
 * [14] mating + tracebacks, [15] best_single replay.  ([10] sums every wave of every launch from its first stamp to its
 * last, so a tier no pair reached still shows cycles there, and nothing else.) */
int abm_ctx_take_work_tiers(abm_ctx *ctx, uint64_t out[32]);
/* Diagnostic build of the single-end kernel only: [0] iterations its scoring rounds ran since the previous call,
 * [1] iterations the same rounds take when each runs to its last row (a round ends early once none of its jobs can
 * still reach a score another job of the read has reached: DESIGN.md 4.1).  Reset by the call. */
int abm_ctx_take_score_iterations(abm_ctx *ctx, uint64_t out[2]);
/* Diagnostic kernel only: device array [n] receiving per-read shader cycles / 1024 (NULL = off). */
int abm_ctx_set_read_cycles(abm_ctx *ctx, uint32_t *d_read_cycles);
/* Paired-end diagnostic kernels only: device array [n][8] (zeroed by the caller) to which the kernels that mate a pair add
 * its shader cycles / 1024 by phase -- probe + narrow, window gather + Hamming, replay, sort + unique, scoring of the
 * pairable entries, mating + tracebacks, best_single, single-end fallback (NULL = off).  A phase whose two stamps come
 * out in the wrong order (the counter has been seen to step back under a wave that is resident for long) adds 0. */
int abm_ctx_set_pair_phases(abm_ctx *ctx, uint32_t *d_pair_phases);

/* Measurement hook: when enabled, every main mapping-kernel launch is bracketed by
 * HIP events recorded on the stream it is launched on (one per single-end batch, abm_ctx_pe_timed_launches() per
 * paired-end batch; the extra launches for reads and ends of more than 1024 bases are not bracketed);
 * take_kernel_time waits for them and returns the number of launches and their summed duration. */
int abm_ctx_set_timing(abm_ctx *ctx, int enable);
int abm_ctx_take_kernel_time(abm_ctx *ctx, uint64_t *launches, double *total_ms);
/* Same, one duration per launch in launch order (paired-end: abm_ctx_pe_timed_launches() per call). */
int abm_ctx_take_kernel_times(abm_ctx *ctx, double *ms_out, uint64_t capacity, uint64_t *launches);

/* Mapping statistics are six counters per struct (src/abismal.cpp:865-895) in
 * up to three structs (pairs, read1, read2: :1034-1037) = 18 x u64.  Sums them
 * over every context in ctxs[] with one RCCL all-reduce (ncclSum over xGMI);
 * counters[k] points at the 18 host values of context k and receives the sum.
 * Contexts that share a device (two replicas on one GPU) are summed on the host instead: a communicator takes a
 * device once. */
int abm_stats_allreduce(abm_ctx *const *ctxs, int n_ctx, uint64_t *const *counters);

/* BGZF input inflated on the device (no reference counterpart: the reference reads its FASTQ through htslib on the host,
 * src/abismal.cpp:150-209).  bgzip and the base-callers write compressed FASTQ as BGZF (SAM specification 4.1):
 * independent gzip members of at most 64 KB whose headers say how long they are -- so a batch of blocks is inflated as a
 * batch of reads is mapped, one wavefront per block (RFC 1951: stored, fixed and dynamic blocks; the member's ISIZE and
 * CRC-32 are checked on the device too).
 * A block descriptor: the member is bytes [at, at + len) of the compressed buffer and its text is bytes
 * [text_at, text_at + text_len) of the text buffer; len and text_len are at most 65536.  Each block gets a status byte. */
typedef struct abm_inflater abm_inflater; /* one stream on one GPU + its grow-only device buffers and pinned staging */
typedef struct { uint64_t at; uint64_t text_at; uint32_t len; uint32_t text_len; } abm_bgzf_block;
enum {
  ABM_INFLATE_OK = 0, /* the block inflated */
  ABM_INFLATE_HEADER, /* not a BGZF header, or a field (XLEN, a subfield, BSIZE, the descriptor) that points outside the block */
  ABM_INFLATE_DATA,   /* an invalid deflate stream: block type 3, stored LEN / NLEN that disagree, over-subscribed or
                         illegally incomplete code lengths, a repeat code with nothing to repeat, literal/length symbols
                         286 / 287, distance symbols 30 / 31, a distance beyond the text so far, a stream past the block's end */
  ABM_INFLATE_SIZE,   /* the text produced is not text_len bytes, or the member's ISIZE is not text_len */
  ABM_INFLATE_CRC     /* checksum mismatch */
};
#define ABM_ERR_INFLATE (-3)
/* Host: walks the headers of `bytes` bytes of BGZF -- one descriptor per block (blocks without text included), the texts
 * laid end to end from 0.  out may be NULL (capacity 0) to count: *n_blocks and *text_bytes are always the file's.  A
 * header that is not BGZF's, or a file that ends inside a header or a block, is an error (< 0) that names the offset;
 * ABM_ERR_CAPACITY if there are more blocks than `capacity`. */
int abm_bgzf_scan(const void *comp, uint64_t bytes, abm_bgzf_block *out, uint64_t capacity, uint64_t *n_blocks, uint64_t *text_bytes);
/* An inflater is independent of any abm_ctx; several on one device run side by side, each on its own stream.  Calls on one
 * inflater are serialised.  Without a HIP device the call fails with a message: the library has no CPU fallback. */
int abm_inflater_create(int device, abm_inflater **out);
void abm_inflater_destroy(abm_inflater *inf);
/* Host buffers (pageable is fine): upload, inflate, copy out; returns when the text is in `text`.
 *   0                every block is ABM_INFLATE_OK
 *   ABM_ERR_INFLATE  the call ran and some block's status is not: the texts of the OK blocks are valid, a failed block's
 *                    range of `text` holds unspecified bytes, nothing outside the blocks' ranges is touched
 *   other < 0        the call itself failed (abm_last_error()): a null pointer, a descriptor whose at + len exceeds
 *                    comp_bytes or whose text_at + text_len exceeds text_bytes (checked before anything is launched), a
 *                    HIP error.  Nothing was written. */
int abm_inflate_bgzf(abm_inflater *inf, const void *comp, uint64_t comp_bytes, const abm_bgzf_block *blocks, uint32_t n_blocks,
                     void *text, uint64_t text_bytes, uint8_t *status);
/* The same with everything resident in HBM (d_* are device pointers, descriptors included), enqueued on `stream` (a
 * hipStream_t; NULL = default stream) and not synchronised, as abm_map_se_device: returns 0 once enqueued, the outcome is
 * d_status.  A descriptor that points outside comp_bytes / text_bytes gets ABM_INFLATE_HEADER from the kernel. */
int abm_inflate_bgzf_device(abm_inflater *inf, const void *d_comp, uint64_t comp_bytes, const abm_bgzf_block *d_blocks, uint32_t n_blocks,
                            void *d_text, uint64_t text_bytes, uint8_t *d_status, void *stream);

/* Text deflated into BGZF blocks on the device: abm_inflate_bgzf's mirror image (no reference counterpart: the reference
 * compresses its BAM output through htslib on the host, src/abismal.cpp:513-543).  The text is cut every block_bytes
 * (0 = 0xff00, the most a block may hold here) and every piece becomes one BGZF member, one wavefront per member: the
 * 18-byte header with the BC subfield, ONE deflate block -- fixed Huffman codes (RFC 1951 3.2.6) over greedy matches of
 * 4 to 258 bytes at most 32768 back, or a stored block where that would be longer than the piece + 5 bytes -- then CRC-32
 * and ISIZE.  A member is at most its text + 31 bytes.  The members lie end to end; descriptor k says where member k is
 * ([at, at + len) of the output) and which text it holds ([text_at, text_at + text_len)).  No end-of-file block is
 * appended.  The bytes are a function of the text and block_bytes alone: the device, every deflater and
 * abm_deflate_bgzf_host give the same. */
typedef struct abm_deflater abm_deflater; /* one stream on one GPU + its grow-only device buffers and pinned staging */
/* bytes that surely hold the members of text_bytes of text cut every block_bytes (0 = 0xff00; above 0xff00: returns 0
 * with a message in abm_last_error()) */
uint64_t abm_deflate_bgzf_bound(uint64_t text_bytes, uint32_t block_bytes);
/* A deflater is independent of any abm_ctx and of any inflater; several on one device run side by side, each on its own
 * stream.  Calls on one deflater are serialised.  Without a HIP device the call fails with a message. */
int abm_deflater_create(int device, abm_deflater **out);
void abm_deflater_destroy(abm_deflater *def);
/* Host buffers (pageable is fine): upload, deflate, copy out; returns when the members are in out[0, *out_bytes).  blocks
 * may be NULL (blocks_capacity 0); *n_blocks is the number of members.  text_bytes == 0: no member, *out_bytes == 0.
 *   0                 done
 *   ABM_ERR_CAPACITY  out_capacity or blocks_capacity is too small: *out_bytes / *n_blocks say what is needed, nothing
 *                     was written to out or blocks
 *   other < 0         the call itself failed (abm_last_error()): a null pointer or block_bytes above 0xff00 (checked
 *                     before anything is launched), a HIP error */
int abm_deflate_bgzf(abm_deflater *def, const void *text, uint64_t text_bytes, uint32_t block_bytes,
                     void *out, uint64_t out_capacity, uint64_t *out_bytes,
                     abm_bgzf_block *blocks, uint64_t blocks_capacity, uint64_t *n_blocks);
/* The same with everything resident in HBM (d_* are device pointers), enqueued on `stream` (a hipStream_t; NULL = default
 * stream) and not synchronised, as abm_inflate_bgzf_device: returns 0 once enqueued.  d_blocks holds one descriptor per
 * member: ceil(text_bytes / block_bytes) of them.  *d_out_bytes is always what the members take; if that is more than
 * out_capacity nothing at or beyond d_out + out_capacity is written.  The members are encoded in the deflater's own
 * scratch memory, which a later call on the same deflater reuses: order such calls on one stream. */
int abm_deflate_bgzf_device(abm_deflater *def, const void *d_text, uint64_t text_bytes, uint32_t block_bytes,
                            void *d_out, uint64_t out_capacity, uint64_t *d_out_bytes,
                            abm_bgzf_block *d_blocks, void *stream);
/* The same encoder run serially on the calling thread, no device needed: the specification of the device's bytes.
 * Arguments and results as abm_deflate_bgzf. */
int abm_deflate_bgzf_host(const void *text, uint64_t text_bytes, uint32_t block_bytes,
                          void *out, uint64_t out_capacity, uint64_t *out_bytes,
                          abm_bgzf_block *blocks, uint64_t blocks_capacity, uint64_t *n_blocks);

/* FASTQ text parsed on the device: what ReadLoader does to every record on the host (src/abismal.cpp:164-201), for a whole
 * text at once, so that text inflated in HBM becomes the seq_blob / seq_off of abm_map_se_device / abm_map_pe_device
 * without leaving it.  The rules (abm_fastq_core.hpp has them once, for the CLI's host parser, the kernels and
 * abm_fastq_parse_host alike):
 *   lines     only '\n' ends a line; a last line without one counts.  The text begins at a record's first line; line k
 *             belongs to record k / 4, and L lines are (L + 2) / 4 records: a trailing name line without its sequence line
 *             is not a record.  Lines 4j + 2 and 4j + 3 are never looked at.
 *   name      line 4j: the bytes after its first byte up to the first space, tab or end of line; an empty line is
 *             ABM_FASTQ_EMPTY_NAME
 *   sequence  line 4j + 1: 32767 bytes or more are ABM_FASTQ_TOO_LONG; with fewer than min_letters bytes that are not 'N'
 *             (44, or 36 with a short-read index) the read is empty; otherwise trailing 'N's are dropped, then everything
 *             before the first A, C, G or T; nothing left is ABM_FASTQ_NO_BASE
 *   errors    of several, the one on the lowest line is the call's, as the host throws at the first
 * The kernels: newlines counted per tile of ABM_FASTQ_TILE_BYTES, the counts scanned by one workgroup
 * ABM_FASTQ_SCAN_TILES at a time, every newline ranked into its record's line ends, a group of 16 lanes per record for
 * the name's length and the read's range, the read lengths summed and scanned per chunk of ABM_FASTQ_CHUNK_RECORDS, the
 * reads copied.  The outputs are a function of the text and min_letters alone. */
typedef struct abm_fastq_parser abm_fastq_parser; /* one stream on one GPU + its grow-only device buffers and pinned staging */
enum { ABM_FASTQ_OK = 0, ABM_FASTQ_EMPTY_NAME, ABM_FASTQ_TOO_LONG, ABM_FASTQ_NO_BASE };
#define ABM_ERR_FASTQ (-4)
#define ABM_FASTQ_TILE_BYTES 4096
#define ABM_FASTQ_SCAN_TILES 1024
#define ABM_FASTQ_CHUNK_RECORDS 1024
/* n_records: the text's records; blob_bytes: the reads' bytes; max_len: the longest read after trimming; code: ABM_FASTQ_*;
 * line: the error's line, 0-based within the call's text; value: the line's length for ABM_FASTQ_TOO_LONG, else 0.  A
 * record whose sequence line is an error counts as an empty read. */
typedef struct { uint64_t n_records, blob_bytes; uint32_t max_len, code; uint64_t line, value; } abm_fastq_info;
/* the three sizes above as the library was built with them (tests place their texts' edges by them) */
void abm_fastq_sizes(uint32_t *tile_bytes, uint32_t *scan_tiles, uint32_t *chunk_records);
/* A parser is independent of any abm_ctx, inflater and deflater; several on one device run side by side, each on its own
 * stream.  Calls on one parser are serialised.  Without a HIP device the call fails with a message
 * (abm_fastq_parse_host needs none). */
int abm_fastq_parser_create(int device, abm_fastq_parser **out);
void abm_fastq_parser_destroy(abm_fastq_parser *p);
/* Host buffers (pageable is fine): upload, parse, copy out; returns when the outputs are written.  off receives
 * n_records + 1 offsets into blob, the first 0 -- what abm_map_se_batch takes as seq_off -- and so holds rec_capacity + 1
 * entries; name_at[j] is the offset in `text` of record j's first name byte and name_len[j] the name's length (either may
 * be NULL; rec_capacity entries).  *info is written by every call that gets as far as looking at the text.
 *   0                 done
 *   ABM_ERR_FASTQ     the call ran and info->code != 0: info says which line; n_records is still the text's, the outputs
 *                     hold unspecified bytes inside their ranges
 *   ABM_ERR_CAPACITY  n_records > rec_capacity or blob_bytes > blob_capacity: info says what is needed (an error in the
 *                     text included), nothing else was written
 *   other < 0         the call itself failed (abm_last_error()): a null pointer or a text of 2^32 bytes or more (checked
 *                     before anything is launched), a HIP error.  Nothing was written. */
int abm_fastq_parse(abm_fastq_parser *p, const void *text, uint64_t text_bytes, uint32_t min_letters,
                    char *blob, uint64_t blob_capacity, uint64_t *off, uint64_t *name_at, uint32_t *name_len,
                    uint64_t rec_capacity, abm_fastq_info *info);
/* The same with everything resident in HBM (d_* are device pointers, d_text at any byte alignment), enqueued on `stream`
 * (a hipStream_t; NULL = default stream) and not synchronised, as abm_inflate_bgzf_device: returns 0 once enqueued, the
 * outcome is *d_info.  If d_info->n_records > rec_capacity nothing else was written and the other fields of *d_info are 0;
 * otherwise *d_info is complete and d_off, d_name_at, d_name_len are written; bytes of the reads at or beyond
 * d_blob + blob_capacity are left out (blob_bytes says whether there were any).  The line ends and read lengths are kept in
 * the parser's own scratch memory, which a later call on the same parser reuses: order such calls on one stream. */
int abm_fastq_parse_device(abm_fastq_parser *p, const void *d_text, uint64_t text_bytes, uint32_t min_letters,
                           char *d_blob, uint64_t blob_capacity, uint64_t *d_off, uint64_t *d_name_at,
                           uint32_t *d_name_len, uint64_t rec_capacity, abm_fastq_info *d_info, void *stream);
/* The same rules run serially on the calling thread, no device needed: the specification of the device's bytes.
 * Arguments and results as abm_fastq_parse. */
int abm_fastq_parse_host(const void *text, uint64_t text_bytes, uint32_t min_letters,
                         char *blob, uint64_t blob_capacity, uint64_t *off, uint64_t *name_at, uint32_t *name_len,
                         uint64_t rec_capacity, abm_fastq_info *info);

#ifdef __cplusplus
}
#endif
#endif /* ABISMAL_AMD_H */
