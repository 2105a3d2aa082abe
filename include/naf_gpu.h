/*
 * naf_gpu.h -- C-ABI of libnaf_gpu.so: the MI355X (gfx950) implementation of the ennaf/unnaf hot path.
 *
 * The reference (KirillKryukov/naf v1.3.0) has no plugin/FFI API; its hot path is reached through
 * three internal seams, and each entry point below replaces one of them (paths are relative to the
 * reference tree):
 *
 *   naf_gpu_zstd_decompress   <- ZSTD_decompress / ZSTD_decompressStream call sites
 *                                unnaf/src/input.c:155,183,212,230 (one-shot sections) and
 *                                input.c:262-285,368,399,426, output.c:646 (streamed sequence/quality)
 *   naf_gpu_unnaf             <- print_fasta / print_fastq / print_dna / print_sequences / print_4bit
 *                                unnaf/src/output.c:608-674, output-fastq.c:100-149, output.c:457-512,
 *                                output-sequences.c:60-116, output.c:266-292 (incl. write_4bit_as_fasta
 *                                output.c:445, mask_dna_buffer output.c:295, print_dna_split_into_lines :339)
 *   naf_gpu_ennaf             <- process() + the seq/name/comm/qual writers + compress() + section writer
 *                                ennaf/src/process.c:586-615 (parsers :314-544), process.c:12-57,
 *                                encoders.c:30-146, compressor.c:119-147, ennaf.c:538-589
 *   naf_gpu_zstd_compress     <- compress()/compressor_end_stream(), ennaf/src/compressor.c:64-147
 *
 * Conventions: extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0
 * on success or a negative NAF_GPU_E* code; naf_gpu_last_error(ctx) gives the text (for parity with
 * the reference's die() strings where the reference defines one).  One ctx per device and per host
 * thread; calls on a ctx are serialised on its HIP stream.  "d_" pointers are device (HBM) addresses,
 * "h_" pointers are host addresses.  "d_" pointers may have any alignment; a call writes only inside
 * [d_out, d_out + capacity), its result depends only on [d_src, d_src + len), and with NAF_GPU_ECAP
 * *out_len (where the call has one that reports it) is the size of the whole result.  There is NO CPU fallback: without a usable gfx950 device
 * naf_gpu_init fails with NAF_GPU_ENODEV.
 */
#ifndef NAF_GPU_H
#define NAF_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct naf_gpu_ctx naf_gpu_ctx;

enum {
    NAF_GPU_OK = 0,
    NAF_GPU_ENODEV = -1,     /* no HIP device / wrong architecture */
    NAF_GPU_EHIP = -2,       /* HIP runtime error (text in last_error) */
    NAF_GPU_ENOMEM = -3,     /* device workspace allocation failed */
    NAF_GPU_EFORMAT = -4,    /* malformed .naf container (reference: die() in input.c:31-77) */
    NAF_GPU_EZSTD = -5,      /* corrupt / unsupported zstd frame */
    NAF_GPU_ECAP = -6,       /* output capacity too small; required size is reported */
    NAF_GPU_EINPUT = -7,     /* input text rejected (reference die() messages of process.c) */
    NAF_GPU_EARG = -8,
    NAF_GPU_EINTERNAL = -9   /* a state the library's own reasoning rules out (text in last_error) */
};

/* sequence types (NAF header byte; ennaf.c:52, unnaf.c:27) and text formats (ennaf.c:47) */
enum { NAF_SEQ_DNA = 0, NAF_SEQ_RNA = 1, NAF_SEQ_PROTEIN = 2, NAF_SEQ_TEXT = 3 };
enum { NAF_FMT_AUTO = 0, NAF_FMT_FASTA = 1, NAF_FMT_FASTQ = 2 };
/* unnaf output types that produce sequence text (unnaf.c:16-24) */
enum { NAF_OUT_DEFAULT = -1, NAF_OUT_FASTA = 0, NAF_OUT_FASTQ = 1, NAF_OUT_SEQ = 2, NAF_OUT_SEQUENCES = 3, NAF_OUT_4BIT = 4 };

/* ---- context ---------------------------------------------------------------------------------- */
int         naf_gpu_init(int device, naf_gpu_ctx **ctx);
void        naf_gpu_shutdown(naf_gpu_ctx *ctx);
const char *naf_gpu_strerror(int code);
const char *naf_gpu_last_error(const naf_gpu_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. the framework's current stream).  NULL = HIP's default
 * (null) stream, as in the HIP API.  Until called, the ctx uses a private non-blocking stream. */
int         naf_gpu_set_stream(naf_gpu_ctx *ctx, void *hip_stream);
int         naf_gpu_synchronize(naf_gpu_ctx *ctx);
/* Pre-size the internal scratch arena (otherwise grown on demand; growth synchronises).  The contexts of the side chains
 * (side sections, a FASTQ's quality stream, the chains behind an encode's split) get an eighth of `bytes` each, at most
 * 4 GiB.  A whole call (unnaf, unnaf_range, ennaf) that had to grow an arena leaves it as ONE allocation when it returns:
 * the growing call pays, the call after it is already in steady state. */
int         naf_gpu_reserve(naf_gpu_ctx *ctx, size_t bytes);

/* ---- device memory for hosts that do not link HIP themselves (the C CLIs) ---------------------------- */
int  naf_gpu_malloc(naf_gpu_ctx *ctx, size_t bytes, void **d_ptr);
int  naf_gpu_free(naf_gpu_ctx *ctx, void *d_ptr);
/* free / total device memory as the runtime sees it now (the hosts size their chunks of an input larger than HBM with it);
 * the scratch arenas of the context (its own and those of its side chains) count as used: naf_gpu_release_scratch gives them back */
int  naf_gpu_mem_info(naf_gpu_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
int  naf_gpu_release_scratch(naf_gpu_ctx *ctx);
int  naf_gpu_host_alloc(naf_gpu_ctx *ctx, size_t bytes, void **h_pinned);
int  naf_gpu_host_free(naf_gpu_ctx *ctx, void *h_pinned);
int  naf_gpu_upload(naf_gpu_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);     /* async on the stream */
int  naf_gpu_download(naf_gpu_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);   /* returns after completion */
int  naf_gpu_download_async(naf_gpu_ctx *ctx, void *h_pinned_dst, const void *d_src, size_t bytes);   /* async on the stream; pair with naf_gpu_synchronize */
int  naf_gpu_copy(naf_gpu_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);         /* device -> device, async on the stream */

/* ---- the collective of the decode path (BASELINE configs[3]: "per-GPU frame ranges, gather") ----------------
 * One process, one context per GPU (what the C hosts do under NAF_GPUS=0,1,...): ctx k decodes its byte range of the text with
 * naf_gpu_unnaf_range on its own device; this call brings the ranges together in d_dst on dst's device -- every source pushes
 * its range over its own xGMI link (peer copy on the source's stream, behind its decode), dst's stream waits for all of them.
 * srcs[k] may be dst itself (its range is copied in place, or left where it is when d_src[k] already lies at its offset).
 * Decision on RCCL (north_star names "an RCCL gather over xGMI"): between the GPUs of ONE process a gather-to-root is N - 1
 * point-to-point pushes whatever library issues them, bound by the root's xGMI ingress (7 links x ~153 GB/s) -- this entry
 * issues exactly those and libnaf_gpu.so stays free of a communicator.  Jobs of one PROCESS per GPU (torch.distributed; bench.py
 * and the tests) do the same exchange as one group of RCCL send/recv (naf_amd/shard.py: gather_ranges).  When the consumer is the
 * HOST (a file, a pipe), no gather between GPUs is wanted at all: every GPU downloads its range over its own PCIe link
 * (naf_gpu_write_file / naf_gpu_download_async per context -- unnaf.c under NAF_GPUS). */
int  naf_gpu_gather_ranges(naf_gpu_ctx *dst, void *d_dst, naf_gpu_ctx *const *srcs, const void *const *d_src,
                           const uint64_t *dst_off, const size_t *len, int n);

/* File <-> HBM through pinned staging on several host threads (io.hip; NAF_GPU_IO_THREADS, default 8): what the reference does with
 * fread / fwrite of 16 KiB (ennaf/src/process.c:143-150, unnaf/src/files.c).  fd must support pread / pwrite (a regular file); the
 * calls return when the transfer is complete.  The copies run on the ctx stream, in order behind whatever was queued there (the
 * kernels that make d_src). */
int  naf_gpu_read_file(naf_gpu_ctx *ctx, int fd, uint64_t file_off, size_t len, void *d_dst);
int  naf_gpu_write_file(naf_gpu_ctx *ctx, int fd, uint64_t file_off, const void *d_src, size_t len);
/* The same for a descriptor that takes its bytes in order (a pipe, a terminal, /dev/null, `>>`): write() from the calling thread, the
 * next chunks already on the link.  The reference's counterpart is fwrite to stdout (unnaf/src/output.c:640-651). */
int  naf_gpu_write_fd(naf_gpu_ctx *ctx, int fd, const void *d_src, size_t len);

/* Byte histogram of a device buffer (unnaf --charcount over the --seq text, output.c:515-605). */
int  naf_gpu_histogram(naf_gpu_ctx *ctx, const void *d_buf, size_t n, uint64_t counts[256]);

/* ---- zstd ----------------------------------------------------------------------------------------- */
/* Decode one or more concatenated zstd frames (RFC 8878, no dictionaries) resident in HBM.
 * has_magic = 0: the first frame lacks its 4-byte magic, exactly as stored inside a .naf section
 * (compressor.c:150-173 strips it, unnaf utils.c:144-150 re-adds it).  *out_len receives the decoded
 * size; with NAF_GPU_ECAP it receives the required size. */
int  naf_gpu_zstd_decompress(naf_gpu_ctx *ctx, const void *d_src, size_t src_len, int has_magic,
                             void *d_dst, size_t dst_cap, size_t *out_len);

/* Compress d_src into ONE zstd frame made of independently coded blocks (single frame: SURVEY.md R1).
 * level <= 1: entropy-only blocks (Huffman literals, RLE, raw), Huffman weights written directly wherever the format allows
 * (up to 128 weights); level >= 2 adds the LZ stage (matches inside a block, coded with the predefined FSE sequence tables)
 * and FSE-codes the Huffman weights when that is smaller.  Blocks never depend on each other at any level.
 * dst_cap must be at least naf_gpu_zstd_compress_bound(src_len); less is NAF_GPU_ECAP and nothing is written. */
int  naf_gpu_zstd_compress(naf_gpu_ctx *ctx, const void *d_src, size_t src_len, int level,
                           void *d_dst, size_t dst_cap, size_t *out_len);
size_t naf_gpu_zstd_compress_bound(size_t src_len);

/* ---- unnaf ------------------------------------------------------------------------------------------ */
typedef struct {
    int      out_type;          /* NAF_OUT_* ; DEFAULT = FASTQ if the archive has quality else FASTA */
    int      use_mask;          /* 0 = --no-mask */
    int64_t  line_length;       /* <0: use the stored value; >=0: --line-length N (0 = no wrapping) */
} naf_gpu_unnaf_opts;

typedef struct {
    int      version, seq_type, flags;
    uint8_t  separator;
    uint64_t line_length, n_sequences;
    uint64_t title_off, title_len;
    uint64_t orig_size[6], comp_size[6], payload_off[6];   /* ids, comments, lengths, mask, sequence, quality */
} naf_gpu_header;

/* Parse the container framing of an archive resident in HBM (header bytes are pulled to the host). */
int  naf_gpu_parse_header(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, naf_gpu_header *hdr);
/* Same for an archive in host memory (used by the CLI before upload). */
int  naf_gpu_parse_header_host(const void *h_naf, size_t naf_len, naf_gpu_header *hdr, char errbuf[128]);

/* Exact size of the text naf_gpu_unnaf will produce (runs the small-section decode + offset scans). */
int  naf_gpu_unnaf_size(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                        size_t *out_len);
/* Archive in HBM -> FASTA/FASTQ/... text in HBM.  Bit-exact with reference unnaf on the same archive. */
int  naf_gpu_unnaf(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                   void *d_out, size_t out_cap, size_t *out_len);
/* Multi-GPU sharding: produce only output bytes [out_begin, out_end) of the full text into d_out
 * (d_out[0] = byte out_begin).  Only the zstd blocks that feed that byte range are decoded. */
int  naf_gpu_unnaf_range(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                         uint64_t out_begin, uint64_t out_end, void *d_out, size_t out_cap, size_t *out_len);

/* ---- unnaf: records and regions by number, id or range ---------------------------------------------------
 * A .naf has no index and the reference's unnaf is one sequential pass (it has no call site for any of this); here the record
 * tables are made on the device per call, so a selection costs the side sections plus the zstd blocks behind the bases it names.
 * A segment is bases [begin, end) of a record, 0-based; begin = 0 with end = NAF_GPU_WHOLE is the record as stored. */
typedef struct { uint64_t record, begin, end; } naf_gpu_segment;
#define NAF_GPU_WHOLE UINT64_MAX

/* ids -> record numbers.  h_ids: n_ids zero-terminated strings laid end to end in HOST memory (ids_bytes in all).
 * records[k] = number of the FIRST record (archive order) whose id equals string k byte for byte, or UINT64_MAX.
 * NAF_GPU_EARG on an archive without an ids section. */
int  naf_gpu_unnaf_find(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_ids, size_t ids_bytes, size_t n_ids,
                        uint64_t *records);
/* Lengths and text offsets of records [first, first + count) under opts, into host arrays: n_bases (count entries, may be NULL) and
 * text_off (count + 1 entries; text_off[k] .. text_off[k + 1] is what naf_gpu_unnaf_range takes for record first + k). */
int  naf_gpu_unnaf_record_table(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                                uint64_t first, uint64_t count, uint64_t *n_bases, uint64_t *text_off);
/* The texts of n_segs segments (a HOST array) laid end to end in the order given; segments may repeat, overlap and come in any order.
 * A whole-record segment is exactly the bytes the record occupies in the text of naf_gpu_unnaf under the same opts.  A sub-range is
 *   FASTA:      '>' id ':' begin+1 '-' end '\n', the bases wrapped at the effective line length (wrapping restarts at the
 *               segment's first base; 0 = one line), a final '\n'   (id: the record's entry of the ids section, empty without one)
 *   SEQUENCES:  the bases and '\n'          SEQ: the bases          FASTQ, 4BIT: NAF_GPU_EARG (4BIT also for whole records)
 * with mask, RNA / protein / text handling as for those bases in the whole text.  `end` beyond the record is clamped to its length;
 * after that begin >= end is NAF_GPU_EARG unless the segment is a whole-record one, and so is record >= n_sequences; last_error
 * names the segment.  Bases behind the last record of a malformed archive are not addressable.  n_segs = 0 gives
 * *out_len = 0; too small a capacity gives NAF_GPU_ECAP and the needed size.  The side sections are decoded once per call, the
 * sequence (and quality) stream only in the blocks behind the segments. */
int  naf_gpu_unnaf_select_size(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                               const naf_gpu_segment *segs, size_t n_segs, size_t *out_len);
int  naf_gpu_unnaf_select(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                          const naf_gpu_segment *segs, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len);
/* The same with a strand per segment.  strand: a HOST array of n_segs bytes, 0 = as stored, 1 = the reverse complement of segment k;
 * NULL = all 0, and then (as with all bytes 0) the call is exactly naf_gpu_unnaf_select.  The text of a reverse segment is the text of
 * a record whose bases are the complements of bases [begin, end) read from end - 1 down to begin: complemented per IUPAC (A<>T, C<>G,
 * M<>K, R<>Y, B<>V, D<>H; S W N - stay; U for T in an RNA archive), every base with its own case, mask and line length applied as for
 * a forward segment (wrapping restarts at the first emitted base).  Its header carries "/rc" directly behind the id:
 *   a sub-range '>' id ':' begin+1 '-' end "/rc" (the forward coordinates);  a whole record '>' id "/rc", then the separator and the
 *   stored name if there is one;  an archive without ids: the stored name, then "/rc";  '@' for FASTQ.
 * A whole FASTQ record has its quality string reversed and its '+' line as in the whole text.  A reverse segment of a protein or text
 * archive and a strand byte other than 0 or 1 are NAF_GPU_EARG (last_error names the segment); everything naf_gpu_unnaf_select
 * rejects is rejected the same way.  A reverse segment decodes the blocks its forward twin decodes. */
int  naf_gpu_unnaf_select_stranded_size(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                                        const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len);
int  naf_gpu_unnaf_select_stranded(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                                   const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len);
/* Host only, no device needed: "ID", "ID:a-b", "ID:a-", "ID:a" (1-based, inclusive, commas in numbers ignored).  The LAST ':' splits
 * when only digits, commas and '-' follow it, so ids that contain ':' work; what follows must then be a range with 1 <= a <= b.
 * Returns the id's length and begin / end 0-based half-open ("ID": 0 / NAF_GPU_WHOLE; "ID:a-": a - 1 / NAF_GPU_WHOLE). */
int  naf_gpu_parse_region(const char *text, size_t *id_len, uint64_t *begin, uint64_t *end);

/* ---- unnaf: IUPAC motifs on either strand, searched in the packed stream -------------------------------------
 * The reference has nothing of the kind (its users pipe the whole text into a searcher).  In the 4-bit code "-TGKCYSBAWRDMHVN" a base is
 * a set of nucleotides (A = 8, C = 4, G = 2, T/U = 1, N = 15, '-' = 0): a stored base c matches a pattern letter p if and only if
 * c != 0 && (c & ~p) == 0, and the complement of a code is its nibble with the bits reversed.
 *   Patterns  1 to 32 letters of ACGTU RYSWKM BDHV N, either case; U and T are one letter in DNA and RNA archives alike; '-', the empty
 *             string, more than 32 letters and anything else are rejected.
 *   Matching  pattern letter j against stored base g + j.  A stored ambiguous base matches only letters that contain all of it (stored N:
 *             pattern N only; stored R: R D V N); a gap matches nothing.  Case (the soft mask) plays no part; the mask is not decoded.  A
 *             hit lies inside one record.  Bases behind the last record of a malformed archive and the padding nibble of an
 *             odd stream are never matched.  Every start position is a hit: AAA in a run of ten A gives eight.
 *   Strands   mask 1 = as stored, 2 = reverse, 3 = both.  A reverse hit at [begin, begin + m) means that the reverse complement of those
 *             stored bases matches the pattern; coordinates are always the forward ones, as naf_gpu_unnaf_select_stranded takes them.  A
 *             pattern equal to its own reverse complement, searched on both strands, gives two hits at each place.
 *   Archives  FASTA and FASTQ archives alike; protein and text archives, and an archive without a sequence section, are NAF_GPU_EARG.
 *             An archive without records gives 0 hits.
 *   Order     ascending (record, begin), then pattern number, then strand (0 before 1); the same on every run.
 * A hit is exactly the (record, begin, begin + length of the pattern, strand) that naf_gpu_unnaf_select_stranded takes. */
typedef struct { uint64_t record, begin; uint32_t pattern, strand; } naf_gpu_hit;   /* 24 bytes; end = begin + length of pattern */

/* host only, no device: the 4-bit sets of a pattern and of its reverse complement (rev[j] = fwd[len - 1 - j] with its bits reversed), and
 * its length; entries behind the length are 0.  NAF_GPU_EARG for what is no pattern. */
int  naf_gpu_compile_motif(const char *text, uint8_t fwd[32], uint8_t rev[32], size_t *len);

/* h_patterns: n_patterns (1..16) zero-terminated strings laid end to end in HOST memory.  Records [first, first + count) are searched
 * (count = NAF_GPU_WHOLE: to the last record); only the zstd blocks behind their bases are decoded when the frame allows it.
 * *n_hits is always the whole count; per_pattern (HOST, n_patterns x 2 entries, may be NULL) receives the count of pattern k on strand s
 * at [2 k + s].  d_hits is DEVICE memory of any alignment: with hit_cap too small the call returns NAF_GPU_ECAP and writes nothing.
 * NAF_GPU_EARG (last_error names the pattern number and the offending letter): a string that is no pattern, first > n_sequences, a range
 * past the last record, n_patterns outside 1..16, strands outside 1..3.  A search of more bases than NAF_GPU_LOCATE_PIECE (default 2^31) is
 * decoded and scanned in pieces of whole records; the result does not depend on the piece size. */
int  naf_gpu_unnaf_locate_count(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                                int strands, uint64_t first, uint64_t count, uint64_t *n_hits, uint64_t *per_pattern);
int  naf_gpu_unnaf_locate(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                          int strands, uint64_t first, uint64_t count, naf_gpu_hit *d_hits, size_t hit_cap, uint64_t *n_hits);

/* ---- unnaf: IUPAC motifs with mismatches and must-match letters ------------------------------------------------
 * What seqkit locate -m and an off-target screen answer from the text: every place within a budget of mismatches of a pattern.
 *   Patterns  those of naf_gpu_compile_motif, and a run of letters in square brackets must match: GAGTCCGAGCAGAAGAAGAA[NGG], [GAATTC],
 *             [TTTV]NNNNNNNNNNNNNNNNNNNNNNN.  Brackets do not nest and are not empty; there may be several runs; 1 to 32 letters, the
 *             brackets not counted.  Everything else is rejected as there; last_error names the pattern number and the position.
 *   Letters   the exact search's rule: stored code c matches letter set p when c != 0 && (c & ~p) == 0; a position that does not match
 *             is a mismatch.  A stored N under a pattern A is one mismatch; a stored gap under anything is one, pattern N included; a
 *             stored R under R, D, V or N is none.  Case and the mask play no part.
 *   Hit       a start position of pattern k where all of the pattern's letters lie inside one record, no bracketed letter mismatches and
 *             the mismatches among the others number at most max_mismatches[k].  Every start position counts, overlapping ones too.
 *             Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no hit.
 *   Budget    per pattern, 0 to NAF_GPU_LOCATE_MAX_MISMATCHES.  A budget above 0 must be smaller than the pattern's number of unbracketed
 *             letters (or every window would be a hit): NAF_GPU_EARG otherwise.
 *   Strands   as in the exact search: a reverse hit at [begin, begin + m) says that the reverse complement of those stored bases is
 *             within the budget of the pattern; coordinates are the forward ones; a palindrome on both strands gives two hits.
 *   where     bit j set when the pattern's letter j mismatched, j the index in the pattern as written, brackets not counted; on the
 *             reverse strand letter j faces stored base begin + m - 1 - j.  popcount(where) == mismatches.
 *   Order     ascending (record, begin), then pattern number, then strand; the same on every run and for every piece size.
 * With every budget 0 and no brackets the table is naf_gpu_unnaf_locate's, row for row, with mismatches = where = 0. */
#define NAF_GPU_LOCATE_MAX_MISMATCHES 8
typedef struct { uint64_t record, begin; uint32_t pattern, strand; uint32_t mismatches, where; } naf_gpu_near_hit;   /* 32 bytes */

/* host only, no device: naf_gpu_compile_motif for a pattern that may hold brackets; *fixed has bit j set when letter j (brackets not
 * counted) stands in brackets, *len is the number of letters.  NAF_GPU_EARG for what is no pattern; nothing is written then. */
int  naf_gpu_compile_motif_near(const char *text, uint8_t fwd[32], uint8_t rev[32], uint32_t *fixed, size_t *len);

/* As naf_gpu_unnaf_locate_count / naf_gpu_unnaf_locate (the same patterns blob, limits, archives, first / count, pieces through
 * NAF_GPU_LOCATE_PIECE), with h_max_mismatches: n_patterns budgets in HOST memory.  per_pattern (HOST, n_patterns x 2 x 9 entries, may
 * be NULL) receives at [(2 k + s) * 9 + d] the hits of pattern k on strand s with exactly d mismatches.  d_hits is DEVICE memory of any
 * alignment, 32 bytes a hit: with hit_cap too small the call returns NAF_GPU_ECAP, sets *n_hits to the whole count and writes nothing. */
int  naf_gpu_unnaf_locate_near_count(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                                     const uint32_t *h_max_mismatches, int strands, uint64_t first, uint64_t count, uint64_t *n_hits, uint64_t *per_pattern);
int  naf_gpu_unnaf_locate_near(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                               const uint32_t *h_max_mismatches, int strands, uint64_t first, uint64_t count, naf_gpu_near_hit *d_hits, size_t hit_cap, uint64_t *n_hits);

/* ---- unnaf: base composition per record and per window, counted in the packed stream --------------------------
 * What faCount, seqkit fx2tab -g -B and bedtools nuc answer from the text, counted from the 4-bit codes without expanding them.
 *   Rows      window == 0: exactly one row per record, [0, len); an empty record gives a row of zeros.  window == W > 0: a record of len
 *             bases gives ceil(len / W) rows [k W, min((k + 1) W, len)); an empty record gives none.  Any W >= 1 is legal, also one larger
 *             than every record.
 *   Order     ascending (record, begin); the same bytes on every run.  sum(n[0..15]) == end - begin in every row.
 *   Records   [first, first + count), count = NAF_GPU_WHOLE: to the last record.  first > n_sequences, a range past the last record, a
 *             protein or text archive and an archive that stores no sequence are NAF_GPU_EARG, as for naf_gpu_unnaf_locate; an archive
 *             without records gives 0 rows.  FASTA and FASTQ archives alike, DNA and RNA.
 *   Never     Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no row.
 *   cpg       The C lies in the row; the G may lie in the next window of the same record, never in the next record, in the R7 tail or in
 *             the padding nibble.
 *   masked    With NAF_GPU_COMP_MASK and an archive that has a mask section: the bases g of the row with an odd number of mask toggles
 *             <= g, g the base's index in the whole stream -- exactly the lower-case letters of the --sequences text.  Without the flag
 *             or without a mask section it is 0 and the mask section is not decoded.  Any other bit in flags is NAF_GPU_EARG.
 *   d_rows    DEVICE memory of any alignment; exactly 168 * n_rows bytes are written and nothing else.  With row_cap too small the call
 *             returns NAF_GPU_ECAP, sets *n_rows to the whole count and writes nothing.
 *   h_total   HOST, may be NULL: the sum of all rows; its record is the number of records covered, its begin 0, its end their bases.
 * naf_gpu_unnaf_composition_rows needs the lengths section only and decodes no sequence.  More bases than NAF_GPU_COMPOSITION_PIECE
 * (default 2^31) are decoded and counted in pieces of whole records; the result does not depend on the piece size.  Only the zstd blocks
 * behind the records' bases are decoded when the frame allows it. */
typedef struct {
    uint64_t record, begin, end;   /* bases [begin, end) of record `record`, 0-based */
    uint64_t n[16];                /* stored bases per 4-bit code; index = code in "-TGKCYSBAWRDMHVN" (n[1] is U in an RNA archive) */
    uint64_t masked;               /* bases of the row that are lower case in the whole text with the mask applied; 0 without NAF_GPU_COMP_MASK */
    uint64_t cpg;                  /* positions g in [begin, end) with stored base g == C (code 4) and base g + 1 == G (code 2), g + 1 in the SAME record */
} naf_gpu_comp_row;                /* 168 bytes */
enum { NAF_GPU_COMP_MASK = 1 };

/* host only, no device: rows a record of n_bases gives under `window` */
uint64_t naf_gpu_composition_rows_of(uint64_t n_bases, uint64_t window);

int  naf_gpu_unnaf_composition_rows(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t window,
                                    uint64_t first, uint64_t count, uint64_t *n_rows);
int  naf_gpu_unnaf_composition(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t window, int flags,
                               uint64_t first, uint64_t count, naf_gpu_comp_row *d_rows, size_t row_cap,
                               uint64_t *n_rows, naf_gpu_comp_row *h_total);

/* ---- unnaf: quality statistics per read and per cycle, counted in the quality stream -----------------------------
 * What seqkit fx2tab -q, seqkit stats -a and FastQC's per-base quality answer from the FASTQ text, counted from the stored quality codes
 * without composing that text.  Two tables of the same row, a histogram of the byte values and a total; all arithmetic is integer
 * arithmetic, and the rows are the same bytes on every run and for every piece size.
 *   Error table   naf_gpu_quality_error_table: tab[b] = 2^32 for b < 33, round_half_up(2^32 * 10^(-(b - 33) / 10)) for b >= 33 (0 from
 *                 b = 133 on): the error probability of Phred+33 code b times 2^32.  Integer literals in the library, not pow at run
 *                 time: tab[33] = 4294967296, tab[43] = 429496730, tab[53] = 42949673, tab[73] = 429497, tab[126] = 2; entries 33..126
 *                 sum to 20882629606.  Sums of it (ee) are taken mod 2^64; no row of fewer than 2^32 codes can wrap.
 *   Records       [first, first + count), count = NAF_GPU_WHOLE: to the last record.  first > n_sequences and a range past the last
 *                 record are NAF_GPU_EARG, as for naf_gpu_unnaf_composition; an archive without a quality section is NAF_GPU_EARG
 *                 ("no quality" in last_error).  Any sequence type is accepted, protein and text included: the lengths and the quality
 *                 section are all that is decoded, never the sequence or the mask (an archive with qualities whose sequence section was
 *                 cut out is NAF_GPU_EARG: its lengths have nothing to be held against).  An archive without records gives 0 rows.
 *   Record table  exactly one row per record, ascending: key = the record's number, n = its length.  An empty read gives n = 0, sum = 0,
 *                 ee = 0, min = 255, max = 0.  d_rec_rows == NULL: the table is not wanted; rec_cap is ignored, *n_records is still set.
 *   Cycle table   cycle_bin = W >= 1: ceil(maxlen / W) rows, maxlen the longest SELECTED record (0 rows when all of them are empty);
 *                 row k holds every quality code of every selected record whose 0-based position in its read lies in [k W, (k + 1) W).
 *                 cycle_bin = 0: no cycle table, *n_cycle_rows = 0.  d_cycle_rows == NULL with W > 0: the table is not wanted
 *                 (*n_cycle_rows is still set).  Both tables NULL is legal: h_hist and h_total are then all that is made.
 *   h_hist        HOST, may be NULL: the count per byte value over the selected records.
 *   h_total       HOST, may be NULL: the sum over the selected records; its key is the number of records covered, its min and max are
 *                 taken over all their codes.
 *   Capacity      the d_* pointers are DEVICE memory of any alignment; exactly 56 * rows bytes of each wanted table are written and
 *                 nothing else.  If either wanted table's capacity is too small the call returns NAF_GPU_ECAP, sets both counts to the
 *                 whole sizes and writes nothing to either table.
 *   Malformed     a quality stream shorter than the bases of the records is NAF_GPU_EFORMAT ("corrupted quality").  Bytes behind the
 *                 last record's last code are in no row and not in h_hist.
 *   Pieces        more quality bytes than NAF_GPU_QUALITY_PIECE (default 2^31) are decoded and counted in pieces of whole records; the
 *                 result does not depend on the piece size.  Only the zstd blocks behind the selected records are decoded when the
 *                 frame allows it; a frame of dependent blocks is decoded whole once.
 * naf_gpu_unnaf_quality_rows needs the lengths section only; no quality byte is decoded.  All 256 byte values are legal codes.
 * TRACE=1: "[quality] records R cycle rows C pieces P quality bytes decoded X of Y lds bins K global bins G" per counting call. */
typedef struct {
    uint64_t key;            /* record table: the record's number.  cycle table: the bin's number k; the bin holds read positions [k W, (k+1) W) */
    uint64_t n;              /* quality codes counted in the row */
    uint64_t sum;            /* sum of their byte values (raw bytes, no offset taken off) */
    uint64_t ee;             /* sum of naf_gpu_quality_error_table()[byte]: expected errors times 2^32 */
    uint64_t n_q20, n_q30;   /* codes with byte >= 33 + 20, byte >= 33 + 30 */
    uint32_t min, max;       /* smallest / largest byte of the row; a row with n == 0 has min = 255, max = 0 */
} naf_gpu_qual_row;          /* 56 bytes */

/* host only, no device */
int  naf_gpu_quality_error_table(uint64_t tab[256]);
int  naf_gpu_unnaf_quality_rows(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t cycle_bin, uint64_t first, uint64_t count,
                                uint64_t *n_records, uint64_t *n_cycle_rows);
int  naf_gpu_unnaf_quality(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t cycle_bin, uint64_t first, uint64_t count,
                           naf_gpu_qual_row *d_rec_rows, size_t rec_cap, naf_gpu_qual_row *d_cycle_rows, size_t cycle_cap,
                           uint64_t *n_records, uint64_t *n_cycle_rows, uint64_t h_hist[256], naf_gpu_qual_row *h_total);

/* ---- unnaf: runs of a base class and soft-masked intervals per record, listed from the packed stream ------------------
 * What seqtk cutN -g, twoBitInfo -nBed and seqtk hrun answer from the text -- where the assembly gaps, the contigs inside the scaffolds,
 * the homopolymers and the soft-masked intervals lie -- as a table of intervals of unknown length, made without expanding the codes.
 *   Class     `set` has bit c set for 4-bit code c of "-TGKCYSBAWRDMHVN".  Membership is LITERAL: a stored N is in {N} and a stored R is
 *             not -- unlike the containment rule of naf_gpu_unnaf_locate, where a pattern N matches every stored base.
 *             naf_gpu_parse_base_class takes letters of ACGTU RYSWKM BDHV N and '-', either case, U = T; a leading '^' complements the
 *             set within the sixteen codes.  The empty string, a bare "^" and any other character are NAF_GPU_EARG.
 *   Run       a maximal stretch of consecutive bases of ONE record whose codes are all in `set`, with end - begin >= min_len.  A record's
 *             end always ends a run: a run that reaches the last base of record r and one that starts at base 0 of the next non-empty
 *             record are two rows, however many empty records lie between them.  code = the code of the run's first base.
 *   EACH      NAF_GPU_RUNS_EACH: every code of `set` is a class of its own; a run is then a maximal stretch of one and the same code (a
 *             homopolymer for set = ACGT) and code is that code.
 *   MASKED    NAF_GPU_RUNS_MASKED: runs of bases g that have an odd number of mask toggles <= g, g the base's index in the whole stream
 *             -- exactly the lower-case letters of the --sequences text --, split at record ends in the same way; code = 0.  `set` must
 *             be 0 and EACH absent (NAF_GPU_EARG otherwise).  An archive without a mask section gives 0 runs.  Neither the sequence nor
 *             the quality section is decoded.  Everything is defined by parity, so equal toggles of a foreign archive cancel.
 *   Never     Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no run,
 *             also for a `set` that holds '-' (code 0).
 *   Errors    NAF_GPU_EARG, last_error saying which: set == 0 without MASKED; min_len == 0; unknown flag bits; first > n_sequences or a
 *             range past the last record, as for naf_gpu_unnaf_composition; protein and text archives; an archive that stores no
 *             sequence (for MASKED too: its lengths have nothing to be held against).  An archive without records gives 0 runs.
 *   Order     ascending (record, begin); the same bytes on every run and for every piece size.
 *   Outputs   *n_runs is always the whole count; *n_bases (may be NULL) the sum of end - begin.  d_runs is DEVICE memory of any
 *             alignment; exactly 32 * n_runs bytes are written and nothing else.  With run_cap too small the call returns NAF_GPU_ECAP,
 *             sets *n_runs and writes nothing.
 *   Pieces    more bases than NAF_GPU_RUNS_PIECE (default 2^31) are decoded and swept in pieces of whole records, so no run crosses a
 *             piece; the result does not depend on the piece size.  Only the zstd blocks behind the records are decoded when the frame
 *             allows it.  The tables of run starts and ends of a piece live in the context's scratch arena (at the worst one of each per
 *             two bases; per base with EACH at min_len 1): when it cannot hold them the call returns NAF_GPU_ENOMEM and last_error
 *             names NAF_GPU_RUNS_PIECE.
 * A run is exactly the (record, begin, end) that naf_gpu_unnaf_select takes: the runs of ^N, selected, are a scaffold's contigs.
 * TRACE=1: "[runs] runs R candidates K pieces P sequence bytes decoded X of Y mask toggles T" per call that reaches the records. */
typedef struct { uint64_t record, begin, end; uint32_t code, reserved; } naf_gpu_run;   /* 32 bytes; reserved = 0 */
enum { NAF_GPU_RUNS_EACH = 1, NAF_GPU_RUNS_MASKED = 2 };

/* host only, no device */
int  naf_gpu_parse_base_class(const char *text, uint16_t *set);

int  naf_gpu_unnaf_runs_count(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint16_t set, int flags, uint64_t min_len,
                              uint64_t first, uint64_t count, uint64_t *n_runs, uint64_t *n_bases);
int  naf_gpu_unnaf_runs(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint16_t set, int flags, uint64_t min_len,
                        uint64_t first, uint64_t count, naf_gpu_run *d_runs, size_t run_cap, uint64_t *n_runs, uint64_t *n_bases);

/* ---- unnaf: k-mer spectrum per record or per selection, counted in the packed stream -------------------------------
 * What jellyfish count -m K, tetranucleotide frequencies per contig, codon and hexamer usage answer from the text: exact dense counts of
 * all 4^K k-mers, K = 1 .. 12, made without composing that text.  All arithmetic is integer adds.
 *   Index       A = 0, C = 1, G = 2, T/U = 3, two bits a base; the FIRST base is the most significant, so ascending index is the
 *               lexicographic order of the k-mer strings.  A table has 4^K uint64_t counters.  naf_gpu_kmer_index takes 1 .. 12 letters of
 *               ACGTU in either case (anything else: NAF_GPU_EARG) and gives K and the index -- with canonical != 0 the smaller of the
 *               index and that of the reverse complement; naf_gpu_kmer_text writes the K letters (T, never U) and a 0 byte, and is
 *               NAF_GPU_EARG for K outside 1 .. 12 or index >= 4^K.
 *   Counted     Position g of record r is counted if and only if bases g .. g + K - 1 all lie in record r and each is stored as exactly
 *               A, C, G or T/U (codes 8, 4, 2, 1 of "-TGKCYSBAWRDMHVN").  Any other stored code -- N, an ambiguity code, the gap --
 *               invalidates every k-mer that covers it.  Case (the soft mask) plays no part and the mask section is never decoded.  A
 *               record shorter than K gives nothing.  Every start position counts: AAA in ten A gives eight.
 *   Never       Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no k-mer.
 *   CANONICAL   NAF_GPU_KMER_CANONICAL: each counted k-mer adds to min(index, index of its reverse complement); every other bin stays 0.
 *               A k-mer equal to its own reverse complement (even K only) counts once per occurrence, not twice.
 *   PER_RECORD  NAF_GPU_KMER_PER_RECORD: one table per record of [first, first + count), laid end to end in record order: table i is at
 *               d_counts + i * 4^K; an empty or too-short record gives a table of zeros.  d_rows (may be NULL when not wanted) gets one
 *               naf_gpu_kmer_row per record, at any alignment: begin = 0, end = the length, positions = max(len - K + 1, 0), counted =
 *               the sum of the record's table.  Without the flag there is one table for all selected records (an empty selection: one
 *               table of zeros), *n_rows = 1, d_rows is ignored; k-mers never span two records either way.
 *   h_total     HOST, may be NULL: record = the records covered, begin = 0, end = their bases, positions and counted summed.
 *   Records     [first, first + count), count = NAF_GPU_WHOLE: to the last record.  Errors and archive kinds are those of
 *               naf_gpu_unnaf_composition: first > n_sequences, a range past the last record, protein archives, text archives and
 *               archives that store no sequence are NAF_GPU_EARG; an archive without records gives zero tables (*n_rows = 0).
 *   Arguments   NAF_GPU_EARG, last_error saying which: K outside 1 .. 12; unknown flag bits; a d_counts that is not 8-byte aligned.
 *   Capacity    count_cap is in counters, row_cap in rows.  If either wanted table does not fit the call returns NAF_GPU_ECAP, sets
 *               *n_rows and *n_counters to the whole sizes and writes nothing.  Otherwise exactly 8 * n_rows * 4^K bytes and (with
 *               PER_RECORD and a d_rows) 40 * n_rows bytes are written and nothing else; the call zeroes the tables itself.
 *   Pieces      the bytes are the same on every run and for every piece size.  More bases than NAF_GPU_KMERS_PIECE (default 2^31) are
 *               decoded and swept in pieces of whole records; only the zstd blocks behind the records are decoded when the frame allows
 *               it.  NAF_GPU_KMERS_LDS_K (0 .. 7, default 7): the largest K counted in LDS bins; the result does not depend on it.
 * naf_gpu_unnaf_kmers_rows needs the lengths section only and decodes no sequence.
 * TRACE=1: "[kmers] k K rows R pieces P sequence bytes decoded X of Y lds tiles A global tiles B" per counting call that reaches the records. */
typedef struct { uint64_t record, begin, end, positions, counted; } naf_gpu_kmer_row;   /* 40 bytes */
enum { NAF_GPU_KMER_CANONICAL = 1, NAF_GPU_KMER_PER_RECORD = 2 };

/* host only, no device */
int  naf_gpu_kmer_index(const char *kmer, int canonical, unsigned *k, uint64_t *index);
int  naf_gpu_kmer_text(unsigned k, uint64_t index, char out[13]);

int  naf_gpu_unnaf_kmers_rows(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, unsigned k, int flags, uint64_t first, uint64_t count,
                              uint64_t *n_rows, uint64_t *n_counters);
int  naf_gpu_unnaf_kmers(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, unsigned k, int flags, uint64_t first, uint64_t count,
                         uint64_t *d_counts, size_t count_cap, naf_gpu_kmer_row *d_rows, size_t row_cap,
                         uint64_t *n_rows, uint64_t *n_counters, naf_gpu_kmer_row *h_total);

/* ---- unnaf: open reading frames on the six frames of every record, listed from the packed stream --------------------
 * What getorf, NCBI ORFfinder, orfipy and seqkit translate -F answer from the text -- where the open reading frames lie -- as a table of
 * (record, begin, end, strand) rows, made without expanding the codes.  The rows feed naf_gpu_unnaf_translate, which writes their proteins.
 *   Codon set   a uint64_t: bit i is the codon whose index is i under naf_gpu_kmer_index at K = 3 (A = 0, C = 1, G = 2, T/U = 3, the first
 *               base the most significant): TAA = 48, TAG = 50, TGA = 56, ATG = 14.  naf_gpu_parse_codon_set takes comma-separated
 *               three-letter codons, either case, U = T; the IUPAC letters RYSWKM BDHV N expand ("TAR,TGA" is the three standard
 *               stops).  '-', any other character, an empty item, an item of another length and the empty string are NAF_GPU_EARG, and
 *               nothing is written then.
 *   Known       a codon is three consecutive bases of ONE record at offsets o, o + 1, o + 2.  It is known when each is stored as exactly
 *               A, C, G or T/U (codes 8, 4, 2, 1 of "-TGKCYSBAWRDMHVN"); any other stored code -- N, an ambiguity code, the gap -- makes
 *               it unknown, and an unknown codon is never a stop and never a start.  Case (the soft mask) plays no part and the mask
 *               section is never decoded.  A codon that straddles two records does not exist.
 *   Never       Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no codon.
 *   Frames      strand 0: the frame of a codon is o mod 3.  strand 1 is the reverse complement of the record's L bases: the reverse
 *               codon over forward offsets [o, o + 3) reads comp(o + 2) comp(o + 1) comp(o), and its frame is (L - (o + 3)) mod 3.  This is
 *               the "reverse-complement, then frame 1..3" convention of ORFfinder and seqkit, NOT that of EMBOSS (whose -1..-3 count
 *               from the forward offset).  begin and end are always forward offsets, as naf_gpu_unnaf_select_stranded takes them.
 *   Stretch     for one strand and frame of one record, a maximal series of consecutive in-frame codons none of which is a stop -- with
 *               NAF_GPU_ORF_SPLIT_UNKNOWN none of which is unknown either.  It is bounded on each side by such a codon or by the
 *               record's edge: the first forward codon of frame f is at offset f, the last ends at f + 3 floor((L - f) / 3).
 *   ORF         starts == 0: the whole stretch ("stop to stop", getorf -find 0).  starts != 0: from the 5'-most start codon of the
 *               stretch, in reading direction (on strand 1 the start codon with the greatest forward offset), to the stretch's 3' end;
 *               only that longest ORF of a stretch is listed, no nested ones, and a stretch without a start gives none.  The stop codon
 *               is not part of [begin, end); end - begin is a multiple of 3 and at least min_len.  An empty stretch gives nothing.
 *   Row flags   NAF_GPU_ORF_STOP3: a stop codon lies directly behind the 3' end -- [end, end + 3) on strand 0, [begin - 3, begin) on
 *               strand 1.  NAF_GPU_ORF_STOP5: a stop codon lies directly in front of the STRETCH's 5' end.  Without the bit the stretch
 *               was ended there by the record's edge or, with SPLIT_UNKNOWN, by an unknown codon.
 *   Call flags  NAF_GPU_ORF_SPLIT_UNKNOWN; NAF_GPU_ORF_CLOSED: only rows with STOP3.  strands: 1 forward, 2 reverse, 3 both, as in
 *               naf_gpu_unnaf_locate.
 *   Order       ascending (record, begin, end), then strand; the same bytes on every run and for every piece size.
 *   Errors      NAF_GPU_EARG, last_error saying which: stops == 0; starts & stops != 0; min_len == 0; strands outside 1 .. 3; unknown
 *               flag bits.  Archives, first and count are those of naf_gpu_unnaf_composition: protein archives, text archives and
 *               archives that store no sequence are NAF_GPU_EARG, an archive without records gives 0 rows, count = NAF_GPU_WHOLE means
 *               to the last record.
 *   Outputs     *n_orfs is always the whole count; *n_bases (may be NULL) the sum of end - begin; per_frame (may be NULL) the rows per
 *               [3 * strand + frame].  d_orfs is DEVICE memory of any alignment; exactly 32 * n_orfs bytes are written and nothing else.
 *               With orf_cap too small the call returns NAF_GPU_ECAP, sets *n_orfs and writes nothing.
 *   Pieces      more bases than NAF_GPU_ORFS_PIECE (default 2^31) are decoded and swept in pieces of whole records, so no stretch
 *               crosses a piece; only the zstd blocks behind the records are decoded when the frame allows it.  The lists of stops,
 *               starts and record bounds of a piece live in the context's scratch arena (in random sequence an eighth of an entry per
 *               base): when it cannot hold them the call returns NAF_GPU_ENOMEM and last_error names NAF_GPU_ORFS_PIECE.
 * A row is exactly the (record, begin, end, strand) that naf_gpu_unnaf_select_stranded takes: the rows, selected, are the coding texts.
 * TRACE=1: "[orfs] orfs R stretches S stops B pieces P sequence bytes decoded X of Y" per call that reaches the records. */
typedef struct { uint64_t record, begin, end; uint32_t strand; uint16_t frame, flags; } naf_gpu_orf;   /* 32 bytes */
enum { NAF_GPU_ORF_STOP3 = 1, NAF_GPU_ORF_STOP5 = 2 };              /* naf_gpu_orf.flags */
enum { NAF_GPU_ORF_SPLIT_UNKNOWN = 1, NAF_GPU_ORF_CLOSED = 2 };     /* the calls' flags */

/* host only, no device */
int  naf_gpu_parse_codon_set(const char *text, uint64_t *set);

int  naf_gpu_unnaf_orfs_count(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t stops, uint64_t starts, uint64_t min_len, int strands, int flags,
                              uint64_t first, uint64_t count, uint64_t *n_orfs, uint64_t *n_bases, uint64_t per_frame[6]);
int  naf_gpu_unnaf_orfs(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, uint64_t stops, uint64_t starts, uint64_t min_len, int strands, int flags,
                        uint64_t first, uint64_t count, naf_gpu_orf *d_orfs, size_t orf_cap, uint64_t *n_orfs, uint64_t *n_bases);

/* ---- unnaf: segments and ORFs as protein, translated from the packed stream -------------------------------------------
 * What the same tools print behind the table: the amino acids of a list of segments -- ORF rows, locate hits, runs, frames of whole
 * records -- without the nucleotide text ever being written.
 *   Code        naf_gpu_genetic_code.aa[i] is the letter of the codon whose index is i under naf_gpu_kmer_index at K = 3 (the codon sets'
 *               order: ATG = 14, TAA = 48, TGA = 56); '*' is a stop.  naf_gpu_genetic_code_by_id knows NCBI's tables 1 .. 6, 9 .. 16 and
 *               21 .. 26; naf_gpu_genetic_code_parse takes 64 letters 'A' .. 'Z' or '*', either case, in that index order (NOT NCBI's TCAG
 *               order).  Another id, a NULL, a string of another length or with another character is NAF_GPU_EARG, and nothing is written
 *               then.  naf_gpu_genetic_code_stops gives the codon set of the '*' letters: what naf_gpu_unnaf_orfs takes as stops.
 *   Table       naf_gpu_codon_lut: 4096 letters, index (c0 << 8) | (c1 << 4) | c2 of the stored codes of "-TGKCYSBAWRDMHVN" in reading
 *               order.  Three of A, C, G, T/U: aa[..].  No gap and an ambiguity code: the letter all expansions share (GCN is A, TAR is
 *               '*'), else 'X'.  Three gaps: '-'.  Any other codon with a gap: 'X'.  Upper case always; the mask is never decoded.
 *   Segments    segs and strand are HOST arrays with the meaning they have in naf_gpu_unnaf_select_stranded (strand may be NULL), and the
 *               same errors with the segment named in last_error: a record that is not there, begin >= end after clamping unless the
 *               segment is a whole record, a strand byte other than 0 and 1.
 *   Text        always FASTA-shaped; of opts only line_length is used.  Per segment, in the order given: the header line that
 *               naf_gpu_unnaf_select_stranded writes for it in FASTA mode (">id:a-b", ">id:a-b/rc", a whole record's stored header, or
 *               that with "/rc"), then floor(n / 3) letters read from the segment's first base in reading direction -- on strand 1 the
 *               first codon is the reverse complement of forward bases [end - 3, end) --, wrapped at the line length counted in letters
 *               (0: one line) with a final newline.  One or two trailing bases are dropped; fewer than three bases give the header line
 *               alone.  Stops are '*' and nothing is trimmed.
 *   Archives    DNA and RNA (U is stored as T: the same letters), with or without qualities (the header character is '>').  Protein and
 *               text archives and archives that store no sequence are NAF_GPU_EARG.
 *   Outputs     n_segs = 0 gives *out_len = 0.  With out_cap too small the call returns NAF_GPU_ECAP, sets *out_len to the whole size and
 *               writes nothing; otherwise exactly *out_len bytes are written.  Only the zstd blocks behind the segments are decoded.
 * TRACE=1: "[translate] segments S codons C ranges R sequence bytes decoded X of Y" per call that reaches the records. */
typedef struct { char aa[64]; } naf_gpu_genetic_code;

/* host only, no device */
int  naf_gpu_genetic_code_by_id(int ncbi_id, naf_gpu_genetic_code *code);
int  naf_gpu_genetic_code_parse(const char *letters64, naf_gpu_genetic_code *code);
int  naf_gpu_genetic_code_stops(const naf_gpu_genetic_code *code, uint64_t *stops);
int  naf_gpu_codon_lut(const naf_gpu_genetic_code *code, uint8_t lut[4096]);

int  naf_gpu_unnaf_translate_size(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts, const naf_gpu_genetic_code *code,
                                  const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len);
int  naf_gpu_unnaf_translate(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts, const naf_gpu_genetic_code *code,
                             const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len);

/* ---- unnaf: perfect tandem repeats (microsatellites) of period 1 to 16 per record, listed from the packed stream ------
 * What MISA, PERF, pytrf findstr and seqtk hrun (period 1 only) answer from the text -- where (CA)17, (GATA)12 and the poly-A tails lie --
 * as a table of (record, begin, end, motif, period) rows, made without expanding the codes.
 *   Repeat    of period p, 1 <= p <= 16: a maximal interval [begin, end) of bases of ONE record in which every base is stored as exactly
 *             A, C, G or T/U (codes 8, 4, 2, 1 of "-TGKCYSBAWRDMHVN"), x[i] == x[i + p] holds for every begin <= i < end - p, and
 *             end - begin >= 2p.  Case (the soft mask) plays no part and the mask section is never decoded; an N, an ambiguity code or
 *             the gap ends the interval.  Maximal: it cannot be extended by one base on either side; a record's end always ends it, so a
 *             repeat that reaches the last base of record r and one that starts at base 0 of the next non-empty record are two rows.
 *             Two repeats of the same period may overlap by up to p - 1 bases: ACACAGAGAG holds (AC) at [0, 5) and (AG) at [4, 10).
 *   Motif     the first p bases of the repeat: base i (0 = first) at bits 2i and 2i + 1 of `motif`, A = 0, C = 1, G = 2, T/U = 3; the bits
 *             above 2p are 0.  A repeat whose motif is itself a whole power of a shorter word (AAAA at p = 2, ACAC at p = 4) is NOT a row,
 *             whether or not the shorter period is searched, as in MISA and PERF: the interval is exactly the maximal repeat of that
 *             shorter period.
 *   Spec      min_copies[p - 1] = 0: period p is not searched; otherwise >= 2.  naf_gpu_parse_repeat_spec takes MISA's definition syntax,
 *             PERIOD-COPIES pairs joined by commas ("1-10,2-6,3-5"), each period 1 .. 16 at most once, copies 2 .. 2^32 - 1; the word
 *             "misa" stands for 1-10,2-6,3-5,4-5,5-5,6-5.  Everything else is NAF_GPU_EARG and nothing is written then: the empty string,
 *             a period listed twice, period 0 or 17, copies 0 or 1, blanks, a trailing comma.
 *   Filters   copies = floor((end - begin) / p).  A row is kept when copies >= min_copies[p - 1] and end - begin >= min_len.  With
 *             NAF_GPU_REPEATS_WHOLE_UNITS end is cut to begin + copies * p before the min_len test and in the row: what MISA and PERF print.
 *   Class     naf_gpu_repeat_class gives the smallest, in A < C < G < T order from the first base on, of the 2p rotations of the motif
 *             and of its reverse complement, in the encoding of `motif`: MISA groups (CA)n, (AC)n, (TG)n and (GT)n under AC.  A period
 *             outside 1 .. 16 and motif bits above 2p are NAF_GPU_EARG.
 *   Never     Bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no repeat.
 *   Order     ascending (record, begin, period); the same bytes on every run and for every piece size.
 *   Errors    NAF_GPU_EARG, last_error saying which: a spec that searches no period; a min_copies of 1; unknown flag bits; min_len == 0;
 *             first > n_sequences or a range past the last record, as for naf_gpu_unnaf_runs; protein and text archives; an archive
 *             that stores no sequence.  An archive without records gives 0 rows.
 *   Outputs   *n_repeats is always the whole count; *n_bases (may be NULL) the sum of end - begin over the rows, overlaps counted twice;
 *             per_period (may be NULL) the rows of period p at [p - 1].  d_rows is DEVICE memory of any alignment; exactly
 *             32 * n_repeats bytes are written and nothing else.  With row_cap too small the call returns NAF_GPU_ECAP, sets *n_repeats
 *             to the whole count and writes nothing.
 *   Pieces    more bases than NAF_GPU_REPEATS_PIECE (default 2^31) are decoded and swept in pieces of whole records, so no repeat crosses
 *             a piece; only the zstd blocks behind the records are decoded when the frame allows it.  The candidate tables of a piece
 *             (a start and an end per run of continuing bases that the prefilter cannot drop) live in the context's scratch arena: when it
 *             cannot hold them the call returns NAF_GPU_ENOMEM and last_error names NAF_GPU_REPEATS_PIECE.
 * A row's (record, begin, end) is what naf_gpu_unnaf_select takes: the selected text of a row is its motif repeated and cut to its length.
 * TRACE=1: "[repeats] rows R candidates K periods P pieces N sequence bytes decoded X of Y" per call that reaches the records. */
typedef struct { uint64_t record, begin, end; uint32_t motif; uint8_t period, reserved[3]; } naf_gpu_repeat;   /* 32 bytes; reserved = 0 */
typedef struct { uint32_t min_copies[16]; } naf_gpu_repeat_spec;
enum { NAF_GPU_REPEATS_WHOLE_UNITS = 1 };

/* host only, no device */
int  naf_gpu_parse_repeat_spec(const char *text, naf_gpu_repeat_spec *spec);
int  naf_gpu_repeat_class(uint32_t motif, unsigned period, uint32_t *cls);

int  naf_gpu_unnaf_repeats_count(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_repeat_spec *spec, int flags, uint64_t min_len,
                                 uint64_t first, uint64_t count, uint64_t *n_repeats, uint64_t *n_bases, uint64_t per_period[16]);
int  naf_gpu_unnaf_repeats(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_repeat_spec *spec, int flags, uint64_t min_len,
                           uint64_t first, uint64_t count, naf_gpu_repeat *d_rows, size_t row_cap, uint64_t *n_repeats, uint64_t *n_bases,
                           uint64_t per_period[16]);

/* ---- unnaf: quality trimming and filtering of reads, decided in the quality stream -------------------------------------
 * What seqtk trimfq, BBDuk qtrim=rl, vsearch --fastq_maxee and cutadapt -q answer from the text -- which stretch of every read to keep,
 * and which reads to drop -- as a table of (record, begin, end, ee, flags) rows, made from the quality bytes alone: neither the sequence
 * nor the mask is decoded, and any sequence type is accepted.
 *   Score     s(b) = (int64)limit - (int64)tab[b] of a quality byte b: tab is naf_gpu_quality_error_table (error probability times 2^32),
 *             limit the cutoff error rate in the same units, 1 <= limit <= 2^32.  naf_gpu_trim_limit gives tab[33 + phred], the limit of
 *             "trim below Phred Q" (phred <= 93, else NAF_GPU_EARG; host only); a code exactly at the cutoff scores 0.  All arithmetic is
 *             64-bit integer arithmetic; a read of fewer than 2^31 codes cannot overflow.
 *   Stretch   the Phred / Mott rule, which seqtk and BBDuk apply in floating point: of all non-empty intervals [begin, end) of one read,
 *             the one whose score sum is largest and > 0; among equal sums the smallest begin, then the largest end (so codes that score
 *             0 at either end of it are kept).  With no interval of positive sum begin = end = 0.  With this order the rule is an
 *             associative, ordered combine of summaries of neighbouring pieces of a read, so the answer does not depend on where the
 *             kernels cut the stream.
 *   No trim   limit = NAF_GPU_TRIM_NONE: the stretch is [0, n) of every read, so the filters can be used alone.
 *   ee        of a row: the sum of tab[b] over the stretch (expected errors times 2^32), the ee column of naf_gpu_qual_row restricted to
 *             it: (end - begin) * limit - the stretch's score sum (without a limit: computed as if limit were 0, minus the read's total).
 *   Filters   min_len >= 1; max_ee in table units, UINT64_MAX = none.  flags: NAF_GPU_TRIM_SHORT iff end - begin < min_len (an empty
 *             stretch is always short), NAF_GPU_TRIM_ERRORS iff ee > max_ee, NAF_GPU_TRIM_KEPT iff neither.
 *   Rows      exactly one per selected record, ascending; reserved = 0; the same bytes on every run and for every piece size.  d_rows is
 *             DEVICE memory of any alignment; exactly 40 * n_records bytes are written and nothing else.  d_rows == NULL: the totals only.
 *             With row_cap too small the call returns NAF_GPU_ECAP, sets *n_records and writes nothing.
 *   Total     h_total (HOST memory, may be NULL): reads, kept (rows with NAF_GPU_TRIM_KEPT), bases (all codes of the selected reads),
 *             kept_bases and kept_ee (sums of end - begin and of ee over the kept rows), n_short, n_errors (rows with that flag).
 *   Errors    NAF_GPU_EARG, last_error saying which: limit 0, or above 2^32 and not NAF_GPU_TRIM_NONE; min_len 0; an archive with no
 *             quality section; first > n_sequences or a range past the last record, as for naf_gpu_unnaf_quality.  A quality stream
 *             shorter than the bases is NAF_GPU_EFORMAT.  An archive without records gives 0 rows.
 *   Pieces    more quality bytes than NAF_GPU_TRIM_PIECE (default 2^31) are decoded and swept in pieces of whole records.
 * A kept row's (record, begin, end) is what naf_gpu_unnaf_select_reads takes: the trimmed read under its own header line.
 * TRACE=1: "[trim] records R kept K pieces P quality bytes decoded X of Y open tiles T" per call that reaches the records (T: parts of
 * reads that cross a 4096-byte tile of the sweep, joined by a second kernel). */
#define NAF_GPU_TRIM_NONE UINT64_MAX
enum { NAF_GPU_TRIM_KEPT = 1, NAF_GPU_TRIM_SHORT = 2, NAF_GPU_TRIM_ERRORS = 4 };
typedef struct { uint64_t limit, min_len, max_ee; } naf_gpu_trim_opts;
typedef struct { uint64_t record, begin, end, ee; uint32_t flags, reserved; } naf_gpu_trim_row;   /* 40 bytes; reserved = 0 */
typedef struct { uint64_t reads, kept, bases, kept_bases, kept_ee, n_short, n_errors; } naf_gpu_trim_total;

int  naf_gpu_trim_limit(unsigned phred, uint64_t *limit);     /* host only, no device */
int  naf_gpu_unnaf_trim(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_trim_opts *opts, uint64_t first, uint64_t count,
                        naf_gpu_trim_row *d_rows, size_t row_cap, uint64_t *n_records, naf_gpu_trim_total *h_total);

/* The selection of naf_gpu_unnaf_select_stranded for READS: everything that call is, except that a sub-range segment keeps the header
 * line of the whole-record segment of the same strand ('@' or '>' id name; id "/rc" name for strand 1) instead of id ':' begin+1 '-' end,
 * and is therefore legal in FASTQ: bases [begin, end), "+\n", quality bytes [begin, end) -- both reversed, the bases complemented, for
 * strand 1 -- then '\n'.  Whole-record segments are byte-identical to naf_gpu_unnaf_select_stranded's; NAF_OUT_4BIT and a segment with
 * begin >= end after clamping stay NAF_GPU_EARG. */
int  naf_gpu_unnaf_select_reads_size(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                                     const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len);
int  naf_gpu_unnaf_select_reads(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *opts,
                                const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len);

/* ---- unnaf: 3' adapters clipped from reads, decided in the packed sequence stream ---------------------------------------
 * What cutadapt -a, fastp, Trimmomatic ILLUMINACLIP and BBDuk ktrim=r answer from the text -- where the sequencing adapter begins at the 3'
 * end of every read, an adapter that the read's end cuts short included -- as a table of (record, begin, end, adapter, mismatches,
 * overlap, flags) rows, made without expanding the codes.  Integers only: the same bytes on every run and for every piece size.
 *   Adapters  1 .. NAF_GPU_CLIP_MAX_ADAPTERS of them, each m = 1 .. 32 letters of ACGTU RYSWKM BDHV N in either case, U = T, passed as
 *             the locate calls pass patterns (zero-terminated strings one behind the other).  Square brackets, '-' and anything else are
 *             rejected.  A longer adapter is rejected too: of a 3' adapter the first 32 letters decide the same clip points.  Forward
 *             strand only.  The match rule is naf_gpu_unnaf_locate's: a stored code c matches a letter p iff c != 0 && (c & ~p) == 0, so
 *             a stored N matches only an adapter's N and a stored gap matches nothing.  Case (the soft mask) plays no part.
 *   Window    of record r: [begin_r, end_r) in bases of the record.  d_bounds == NULL: the whole record.  Otherwise d_bounds holds one
 *             naf_gpu_trim_row per selected record (DEVICE memory of any alignment, exactly count rows, what naf_gpu_unnaf_trim wrote for
 *             the same first / count) and the window is the row's (begin, end): quality trimming goes first, as in cutadapt, the adapter
 *             is searched in the quality-trimmed stretch, and "the read's end" is end_r.
 *   Candidate a start x, begin_r <= x < end_r, overlaps adapter k in L = min(m_k, end_r - x) letters; d of the adapter's first L letters
 *             mismatch bases x .. x + L.  x is a candidate of k iff L >= min_overlap and d <= budget[k][L].
 *   Budget    h_budget: 33 bytes per adapter, indexed by L.  For every L in min_overlap .. m_k the call requires budget[k][L] < L
 *             (NAF_GPU_EARG otherwise: every place would be a hit).  naf_gpu_clip_budgets fills a table with floor(L * num / den) for
 *             1 <= L <= m, at most L - 1, and 0 elsewhere: cutadapt's -e rate (default 1/10) as a rational (host only; den == 0 and m
 *             outside 1 .. 32 are NAF_GPU_EARG).
 *   Clip      the smallest candidate x over all adapters; at equal x the lowest adapter number.  A later candidate never wins, however
 *             few mismatches it has.  The kept stretch is [begin_r, x); with no candidate [begin_r, end_r).
 *   Rows      exactly one per selected record, ascending.  adapter: its number, or NAF_GPU_CLIP_NO_ADAPTER; mismatches and overlap (d
 *             and L of the clip point) are 0 then.  flags: NAF_GPU_TRIM_SHORT iff end - begin < min_len; NAF_GPU_TRIM_ERRORS iff the
 *             bounds row had it (never without bounds); NAF_GPU_TRIM_KEPT iff neither; NAF_GPU_CLIP_CLIPPED or-ed in iff an adapter was
 *             found.  Expected errors only fall when a stretch gets shorter: a read within max_ee before the clip is within it after, so
 *             nothing is recomputed (and a read that was outside stays dropped, as in cutadapt's order of steps).  d_rows is DEVICE memory
 *             of any alignment; exactly 40 * n_records bytes are written and nothing else.  d_rows == NULL: the totals only.  With
 *             row_cap too small the call returns NAF_GPU_ECAP, sets *n_records and writes nothing.
 *   Total     h_total (HOST memory, may be NULL): reads, clipped (rows with NAF_GPU_CLIP_CLIPPED), kept (rows with NAF_GPU_TRIM_KEPT),
 *             bases (the windows' bases), kept_bases (end - begin over the kept rows), removed_bases (window end - end over all rows),
 *             n_short, n_errors.  per_adapter (HOST, n_adapters x 33, may be NULL): the clips by [adapter][overlap], the table cutadapt
 *             prints.  All are integer sums.
 *   Errors    NAF_GPU_EARG, last_error saying which: no adapters or more than 16; a letter that is no IUPAC code (with its position); an
 *             adapter of 0 or more than 32 letters; min_overlap 0 or above 32; min_len 0; h_budget NULL or a budget that is no smaller
 *             than its overlap; protein and text archives; first > n_sequences or a range past the last record, as for
 *             naf_gpu_unnaf_locate; a bounds row whose record is not first + its number, whose begin > end or whose end > the record's
 *             length (found on the device; nothing is written to d_rows then, *n_records and *h_total are 0).  An archive without
 *             records gives 0 rows; one without a quality section is as good as any: only the sequence stream is read, and of it only
 *             the zstd blocks behind the selected records when the frame allows it.
 *   Pieces    more bases than NAF_GPU_CLIP_PIECE (default 2^31) are decoded and swept in pieces of whole records.
 * A kept row's (record, begin, end) is what naf_gpu_unnaf_select_reads takes: the clipped read under its own header line.
 * TRACE=1: "[clip] adapters A records R clipped C pieces P sequence bytes decoded X of Y" per call that reaches the records. */
#define NAF_GPU_CLIP_MAX_ADAPTERS 16
#define NAF_GPU_CLIP_NO_ADAPTER UINT32_MAX
enum { NAF_GPU_CLIP_CLIPPED = 8 };                                  /* beside NAF_GPU_TRIM_KEPT, _SHORT, _ERRORS in naf_gpu_clip_row.flags */
typedef struct { uint32_t min_overlap; uint64_t min_len; } naf_gpu_clip_opts;
typedef struct { uint64_t record, begin, end; uint32_t adapter, mismatches, overlap, flags; } naf_gpu_clip_row;   /* 40 bytes */
typedef struct { uint64_t reads, clipped, kept, bases, kept_bases, removed_bases, n_short, n_errors; } naf_gpu_clip_total;

int  naf_gpu_clip_budgets(uint64_t num, uint64_t den, unsigned m, uint8_t out[33]);     /* host only, no device */
int  naf_gpu_unnaf_clip(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const char *h_adapters, size_t adapters_bytes, size_t n_adapters,
                        const uint8_t *h_budget /* n_adapters x 33 */, const naf_gpu_clip_opts *opts, uint64_t first, uint64_t count,
                        const naf_gpu_trim_row *d_bounds /* or NULL */, naf_gpu_clip_row *d_rows, size_t row_cap, uint64_t *n_records,
                        naf_gpu_clip_total *h_total, uint64_t *per_adapter /* n_adapters x 33, or NULL */);

/* ---- unnaf: exact duplicates among reads collapsed, decided in the packed sequence stream -------------------------------
 * What seqkit rmdup -s, fastp --dedup, clumpify dedupe, fastx_collapser and vsearch --derep_fulllength answer from the text -- which reads
 * are copies of an earlier read, and how often every sequence occurs (FastQC's duplication levels) -- as a table of (record, begin, end,
 * first, copies, flags, strand) rows, made without expanding the codes.  Integers only: the table is a function of the codes alone, the
 * same bytes on every run, for every value of NAF_GPU_DEDUP_HASH_BITS and whichever order the kernels meet the records in.
 *   Window    of record r: [begin_r, end_r) in bases of the record.  d_bounds == NULL: the whole record.  Otherwise d_bounds holds exactly
 *             count rows of 40 bytes (DEVICE memory of any alignment), the rows naf_gpu_unnaf_trim (bounds_kind NAF_GPU_DEDUP_BOUNDS_TRIM)
 *             or naf_gpu_unnaf_clip (NAF_GPU_DEDUP_BOUNDS_CLIP: that is where the flags word lies) wrote for the same first / count, and the
 *             window is the row's (begin, end).  A record whose bounds row lacks NAF_GPU_TRIM_KEPT takes NO part: in its row first is its
 *             own number, copies is 0, strand 0, and flags, begin and end are the bounds row's as they came.
 *   Class     two records that take part are in one class iff their windows have the same number of bases and the same stored 4-bit code
 *             at every place.  Case (the mask), qualities, ids and names play no part.  Codes are compared literally: a stored N equals
 *             only a stored N, a gap only a gap; U and T are one code.  Empty windows are equal to each other.  With
 *             NAF_GPU_DEDUP_BOTH_STRANDS in opts.flags two records are also in one class when one window is the reverse complement of the
 *             other: the order reversed and every code complemented by reversing its four bits (T=1 <-> A=8, G=2 <-> C=4).
 *   Rows      exactly one per selected record, ascending.  first: the smallest record number of its class; copies: the records in the
 *             class, the same value in every row of it; strand: 0 when the window equals the first's window as stored, 1 when it equals
 *             only its reverse complement (a window equal both ways has 0, the first itself 0, without the flag always 0).  flags of a
 *             record that takes part: NAF_GPU_TRIM_KEPT if it is its class's first, else NAF_GPU_DEDUP_DUPLICATE; the bounds row's
 *             NAF_GPU_CLIP_CLIPPED is carried.  d_rows is DEVICE memory of any alignment; exactly 48 * n_records bytes are written and
 *             nothing else.  d_rows == NULL: the totals only.  With row_cap too small the call returns NAF_GPU_ECAP, sets *n_records and
 *             writes nothing.
 *   Total     h_total (HOST memory, may be NULL): reads (the selected records), considered (those that take part), classes (rows with
 *             NAF_GPU_TRIM_KEPT), duplicates (considered - classes), singletons (classes of one), largest (the largest copies), bases
 *             (the bases of the windows that take part), kept_bases (those of the firsts' windows).
 *   Levels    h_levels (HOST, NAF_GPU_DEDUP_LEVELS counters, may be NULL): the classes by their copies in FastQC's bins -- 1 to 9 each,
 *             then 10-49, 50-99, 100-499, 500-999, 1000-4999, 5000-9999 and 10000 or more.  naf_gpu_dedup_level gives the bin of a count
 *             (host only; copies == 0 is NAF_GPU_EARG).
 *   Errors    NAF_GPU_EARG, last_error saying which: an unknown flag or bounds_kind; NAF_GPU_DEDUP_HASH_BITS above 64; protein and text
 *             archives ("duplicates cannot be collapsed in %s sequences"); first > n_sequences or a range past the last record, as for
 *             naf_gpu_unnaf_clip; a bounds row whose record is not first + its number, whose begin > end or whose end > the record's
 *             length (found on the device; nothing is written to d_rows then, *n_records, *h_total and h_levels are 0).  An archive
 *             without records gives 0 rows; one without a quality section is as good as any other.
 *   No pieces a comparison needs both records resident: the packed bytes behind the selected records are decoded as ONE range and held
 *             for the call (only the zstd blocks behind them where the frame allows it).  The call needs, beside them, per selected
 *             record 16 bytes of hashes, 16 of window, 8 of first, 8 of copies, 6 of flags and, with d_rows, 48 of row; a table of
 *             8-byte slots, the power of two that is at least 2 * considered (64 at the least); and 96 bytes per 4096 bases.  What does
 *             not fit is NAF_GPU_ENOMEM: there is no piece size to set.
 *   Hashes    a window's 128-bit polynomial hash only FINDS candidates: every duplicate is confirmed by comparing the windows' codes,
 *             and records that share a hash without being equal are resolved in further rounds.  NAF_GPU_DEDUP_HASH_BITS=b (0 to 64)
 *             cuts every 64-bit word of the hash to its low b bits, so that different sequences truly share one: the cross-check lever
 *             of the tests; the table does not change by a byte.  A round that resolves nothing is NAF_GPU_EINTERNAL (never seen).
 * A row with NAF_GPU_TRIM_KEPT gives the (record, begin, end) naf_gpu_unnaf_select_reads takes: every distinct read once.
 * TRACE=1: "[dedup] records R considered C classes U rounds J verified V sequence bytes decoded X of Y" per call that reaches the
 * records (J: rounds of insert + compare; V: pairs of windows whose codes were compared). */
enum { NAF_GPU_DEDUP_DUPLICATE = 16 };            /* beside NAF_GPU_TRIM_KEPT, _SHORT, _ERRORS, NAF_GPU_CLIP_CLIPPED in naf_gpu_dedup_row.flags */
enum { NAF_GPU_DEDUP_BOTH_STRANDS = 1 };          /* opts.flags */
enum { NAF_GPU_DEDUP_BOUNDS_TRIM = 0, NAF_GPU_DEDUP_BOUNDS_CLIP = 1 };
#define NAF_GPU_DEDUP_LEVELS 16
typedef struct { uint32_t flags, bounds_kind; } naf_gpu_dedup_opts;
typedef struct { uint64_t record, begin, end, first, copies; uint32_t flags, strand; } naf_gpu_dedup_row;   /* 48 bytes */
typedef struct { uint64_t reads, considered, classes, duplicates, singletons, largest, bases, kept_bases; } naf_gpu_dedup_total;

int  naf_gpu_dedup_level(uint64_t copies, unsigned *level);    /* host only, no device */
int  naf_gpu_unnaf_dedup(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const naf_gpu_dedup_opts *opts, uint64_t first, uint64_t count,
                         const void *d_bounds /* or NULL */, naf_gpu_dedup_row *d_rows, size_t row_cap, uint64_t *n_records,
                         naf_gpu_dedup_total *h_total, uint64_t *h_levels /* NAF_GPU_DEDUP_LEVELS, or NULL */);

/* ---- unnaf: reads screened against the k-mers of a reference archive, decided in the packed sequence stream -------------
 * What bbduk.sh ref=phix.fa k=27, bbduk outm=, bbsplit and fastq_screen answer from the text -- which reads share k-mers with a contaminant
 * (PhiX spike-in, rRNA, host, vector) or, mirrored, with a target -- as a table of (record, begin, end, hits, flags) rows, made without
 * expanding the codes of either archive.  Integers only: the same bytes on every run, for every piece size and for every value of the
 * two levers below.
 *   K         opts.k, 1 to 31.  The key of a k-mer is naf_gpu_kmer_index's index in 64 bits: A = 0, C = 1, G = 2, T/U = 3, two bits a base,
 *             the first base the most significant.  A key never reaches 2^62.
 *   Valid     a k-mer is what naf_gpu_unnaf_kmers counts: K consecutive bases of ONE record, each stored as exactly A, C, G or T/U.  Any
 *             other stored code invalidates every k-mer that covers it; case plays no part (no mask is decoded); bases behind the last
 *             record of a malformed archive and the padding nibble of an odd stream are in no k-mer.
 *   Set       the keys of all valid k-mers of ALL records of the archive at d_ref (DEVICE memory, ref_len bytes; FASTA or FASTQ, DNA or
 *             RNA, U is T), each as min(key, key of its reverse complement) unless NAF_GPU_SCREEN_FORWARD_ONLY is in opts.flags: then as
 *             stored.  A k-mer that would span two reference records is not in the set.  A reference without a valid k-mer -- or
 *             without records -- is legal: no read matches.
 *   Window    of read r: [begin_r, end_r) in bases of the record.  d_bounds == NULL: the whole record.  Otherwise d_bounds holds exactly
 *             count rows (DEVICE memory of any alignment) written for the same first / count, opts.bounds_kind naming their layout:
 *             NAF_GPU_SCREEN_BOUNDS_TRIM (40 bytes, the flags at byte 32: naf_gpu_unnaf_trim's rows, and this call's own),
 *             NAF_GPU_SCREEN_BOUNDS_CLIP (40 bytes, flags at byte 36: naf_gpu_unnaf_clip's) or NAF_GPU_SCREEN_BOUNDS_DEDUP (48 bytes, flags
 *             at byte 40: naf_gpu_unnaf_dedup's).  A record whose bounds row lacks NAF_GPU_TRIM_KEPT takes NO part: its row has hits = 0,
 *             and flags, begin and end are the bounds row's as they came.
 *   Hits      hits_r: the start positions x in [begin_r, end_r - K] whose k-mer is valid and whose key -- the canonical one unless
 *             FORWARD_ONLY -- is in the set.  Every position counts; a k-mer equal to its own reverse complement counts once.
 *   Verdict   a read is matched iff hits_r >= opts.min_hits (at least 1).  A matched read is dropped -- the filter --; with
 *             NAF_GPU_SCREEN_KEEP_MATCHED an unmatched one is dropped instead.
 *   Rows      exactly one per selected record, ascending: a naf_gpu_trim_row with hits where ee stands, so naf_gpu_unnaf_dedup takes
 *             them as NAF_GPU_DEDUP_BOUNDS_TRIM and the chain trim, clip, screen, dedup never leaves the device.  reserved is 0.  flags
 *             of a read that takes part: NAF_GPU_SCREEN_MATCHED iff it matched, NAF_GPU_TRIM_KEPT iff it is kept under the verdict; the
 *             bounds row's NAF_GPU_CLIP_CLIPPED is carried.  d_rows is DEVICE memory of any alignment; exactly 40 * n_records bytes
 *             are written and nothing else.  d_rows == NULL: the totals only.  With row_cap too small the call returns NAF_GPU_ECAP,
 *             sets *n_records and writes nothing.
 *   Total     h_total (HOST memory, may be NULL), integer sums all: reads (the selected records), considered (those that take part),
 *             matched, kept (rows of reads that take part with NAF_GPU_TRIM_KEPT), bases (of the windows that take part), kept_bases,
 *             kmers (the valid start positions in the windows that take part), hit_kmers (those of them that hit); ref_records and
 *             ref_bases (the reference's records and their bases), ref_positions (its valid start positions), ref_kmers (the distinct
 *             keys in the set).
 *   Errors    NAF_GPU_EARG, last_error saying which: k outside 1 to 31; min_hits 0; unknown flag bits; an unknown bounds_kind; a lever
 *             with a value it does not have; a protein or text archive on either side ("reads cannot be screened in %s sequences");
 *             either archive without a sequence section; first > n_sequences or a range past the last record, as for
 *             naf_gpu_unnaf_clip; a bounds row whose record is not first + its number, whose begin > end or whose end > the record's
 *             length (found on the device; nothing is written to d_rows then, *n_records and *h_total are 0).  A reads archive without
 *             records gives 0 rows.
 *   Pieces    both archives are decoded and swept in pieces of whole records of at most NAF_GPU_SCREEN_PIECE bases (default 2^31): of
 *             the reads only the zstd blocks behind the selected records where the frame allows it, the reference whole.  The set lives
 *             in the context's scratch for the call: a table of 8-byte slots, the power of two that is at least 2 * ref_bases (64 at the
 *             least).  When that cannot be had the call returns NAF_GPU_ENOMEM and last_error names the table.
 *   Levers    NAF_GPU_SCREEN_HASH_BITS=b (0 to 64) cuts the hash that chooses a key's slot to its low b bits, so that different keys
 *             truly share probe chains; NAF_GPU_SCREEN_FILTER_BITS=n sets the bits of the prefilter -- a bitmap with one bit per key of
 *             the set, copied into LDS, that answers "not in the set" for most positions of a clean read without a look at the table --
 *             to n, 0 or a power of two from 64 to 2^19 (default 2^18); 0 switches it off and every valid position probes the table.  Left at its default the bitmap is
 *             only used while the set has at most half as many keys as it has bits: a fuller one lets most positions through.
 *             Neither changes the rows or the totals by a byte.
 * A kept row's (record, begin, end) is what naf_gpu_unnaf_select_reads takes.
 * TRACE=1: "[screen] k K ref records R ref kmers U of V slots S filter bits F reads N considered C matched M filtered Q probed P sequence
 * bytes decoded X of Y" per call that reaches the sweeps (U distinct keys of V valid reference positions; Q and P: the valid read
 * positions the prefilter rejected and let through to the table -- the bitmap is a function of the set, so both are the same on every
 * run; X of Y: of the reads' sequence stream). */
enum { NAF_GPU_SCREEN_MATCHED = 32 };             /* beside NAF_GPU_TRIM_KEPT and NAF_GPU_CLIP_CLIPPED in naf_gpu_screen_row.flags */
enum { NAF_GPU_SCREEN_KEEP_MATCHED = 1, NAF_GPU_SCREEN_FORWARD_ONLY = 2 };     /* opts.flags */
enum { NAF_GPU_SCREEN_BOUNDS_TRIM = 0, NAF_GPU_SCREEN_BOUNDS_CLIP = 1, NAF_GPU_SCREEN_BOUNDS_DEDUP = 2 };
typedef struct { uint32_t k, flags, bounds_kind; uint64_t min_hits; } naf_gpu_screen_opts;
typedef struct { uint64_t record, begin, end, hits; uint32_t flags, reserved; } naf_gpu_screen_row;   /* 40 bytes */
typedef struct { uint64_t reads, considered, matched, kept, bases, kept_bases, kmers, hit_kmers, ref_records, ref_bases, ref_positions, ref_kmers; } naf_gpu_screen_total;

int  naf_gpu_unnaf_screen(naf_gpu_ctx *ctx, const void *d_naf, size_t naf_len, const void *d_ref, size_t ref_len, const naf_gpu_screen_opts *opts,
                          uint64_t first, uint64_t count, const void *d_bounds /* or NULL */, naf_gpu_screen_row *d_rows, size_t row_cap,
                          uint64_t *n_records, naf_gpu_screen_total *h_total);

/* ---- ennaf ------------------------------------------------------------------------------------------ */
typedef struct {
    int      format;            /* NAF_FMT_* (AUTO = sniff, process.c:547-583) */
    int      seq_type;          /* NAF_SEQ_* */
    int      no_mask;           /* --no-mask */
    int      strict;            /* --strict */
    int      level;             /* --level: 1 = ids / names / lengths matched inside a block, other streams entropy-coded; >= 2 = every stream
                                 * matched across blocks inside libzstd's window for that level */
    int64_t  line_length;       /* <0: store the longest line; >=0: --line-length N */
    const char *title;          /* --title or NULL */
    int      long_log;          /* --long N (ennaf.c:247-273): window 2^N for the sequence stream; 0 = not given */
} naf_gpu_ennaf_opts;

typedef struct {
    int      format;            /* detected NAF_FMT_* (0 = empty input) */
    uint64_t n_sequences, n_bases, longest_line;
    uint64_t unexpected_id[257], unexpected_comment[257], unexpected_seq[257], unexpected_qual[257];
    uint64_t section_orig[6], section_comp[6];
} naf_gpu_ennaf_report;

size_t naf_gpu_ennaf_bound(size_t text_len);
/* FASTA/FASTQ text in HBM -> complete .naf archive bytes in HBM. */
int  naf_gpu_ennaf(naf_gpu_ctx *ctx, const void *d_text, size_t text_len, const naf_gpu_ennaf_opts *opts,
                   void *d_naf, size_t naf_cap, size_t *naf_len, naf_gpu_ennaf_report *report);

/* ---- ennaf of ONE input on several GPUs (BASELINE configs[4]) ------------------------------------------------
 * The text is cut into consecutive slices, one per GPU ("shard"); every shard runs the same kernels as naf_gpu_ennaf on its
 * slice and the parts are joined into ONE archive with ONE zstd frame per stream, as reference unnaf requires.
 * What the reference carries from chunk to chunk in its static state travels between shards in a small fixed-size record:
 *   - the half-filled byte of the 4-bit packer   `parity` + pending nibble, ennaf/src/encoders.c:30-69, flushed ennaf.c:525-529
 *   - the open soft-mask run                      `mask_on` / `mask_len`,    encoders.c:126-146, flushed ennaf.c:511
 *   - the record a cut falls into                 add_length(),              process.c:424 (FASTA slices may start inside a record)
 *   - n_sequences, seq_size_original, longest_line_length, the unexpected-character tallies (process.c:389-393,424-425)
 * Protocol (the same calls whether the shards are threads of one process or ranks of torch.distributed / MPI):
 *   0. naf_gpu_ennaf_sniff on the start of the text -> format and p0; slices start at p0.
 *      Cuts: FASTA behind any EOL-class byte (naf_gpu_ennaf_find_cut); FASTQ at a line start whose ordinal is a multiple of 4
 *      (naf_gpu_ennaf_count_lines of every nominal slice, prefix sum, naf_gpu_ennaf_find_cut with the lines to skip).
 *   1. every shard: naf_gpu_ennaf_shard_begin(slice) -> naf_gpu_shard_info.            [all-gather the infos]
 *   2. every shard: naf_gpu_ennaf_shard_finish(all infos) -> its parts of the six frames in a device buffer + their sizes.
 *                                                                                      [gather the naf_gpu_shard_pieces]
 *   3. anyone: naf_gpu_ennaf_stitch_plan -> where every part and the framing bytes go; move the bytes (naf_gpu_ennaf_stitch for
 *      buffers one process can address, RCCL send/recv or per-GPU D2H + pwrite otherwise).
 * An error of any shard (strict mode, malformed FASTQ) is reported by every shard's finish with the reference's message and
 * the record numbered across shards. */
enum { NAF_GPU_MAX_SHARDS = 64 };
typedef struct {
    uint32_t shard, n_shards;
    int32_t  format, seq_type;
    uint64_t text_len;
    uint64_t n_sequences, n_bases, longest_line;
    uint64_t lead_bases;                    /* FASTA: bases in front of the slice's first header (they end an earlier shard's record) */
    uint64_t n_ids, n_comments, n_quality;  /* bytes of the slice's ids / comments / quality streams */
    uint64_t mask_changes;                  /* case changes at base positions >= 1 of the slice, the first and the last of them */
    uint64_t mask_first_change, mask_last_change;
    uint8_t  first_base, last_base;         /* post-replacement; valid when n_bases > 0 */
    uint8_t  store_mask, store_quality, pad_[4];
    int32_t  err_kind; uint32_t err_char;   /* 0 = none; see naf_gpu_ennaf_shard_finish */
    uint64_t err_record, err_a, err_b;
    uint64_t unexpected[4][257];            /* id, comment, sequence, quality (process.c:75-96) */
} naf_gpu_shard_info;

typedef struct {
    uint64_t off[6], len[6];                /* this shard's part of each stream's frame inside its piece buffer (ids, comments, lengths, mask, sequence, quality) */
    uint64_t raw[6];                        /* uncompressed bytes behind each part (sequence: bases) */
    uint64_t total;                         /* bytes used in the piece buffer */
} naf_gpu_shard_pieces;

typedef struct {
    uint64_t dst_off, len, src_off;         /* archive offset; source offset inside the shard's piece buffer, or inside `lit` */
    int32_t  shard, stream;                 /* shard < 0: framing bytes from `lit` */
} naf_gpu_stitch_seg;

/* process.c:547-583: format of the text and the offset of its first record.  *format = 0 for an empty / all-space text. */
int  naf_gpu_ennaf_sniff(naf_gpu_ctx *ctx, const void *d_text, size_t text_len, int want_format, int *format, uint64_t *p0);
/* FASTQ: line starts (non-EOL byte behind an EOL-class byte) inside a slice; prev_is_eol: the byte in front of the slice is
 * EOL-class, or the slice starts at p0. */
int  naf_gpu_ennaf_count_lines(naf_gpu_ctx *ctx, const void *d_slice, size_t len, int prev_is_eol, uint64_t *n_line_starts);
/* Where a shard may begin inside a slice: FASTA -- the first byte behind an EOL-class byte; FASTQ -- line start number
 * skip_lines (0-based) of the slice.  *offset = len when the slice holds no such place. */
int  naf_gpu_ennaf_find_cut(naf_gpu_ctx *ctx, const void *d_slice, size_t len, int format, int prev_is_eol, uint64_t skip_lines,
                            uint64_t *offset);
/* Step 1.  format: NAF_FMT_FASTA or NAF_FMT_FASTQ (from the sniff).  The slice must stay in place until the finish. */
int  naf_gpu_ennaf_shard_begin(naf_gpu_ctx *ctx, const void *d_slice, size_t len, const naf_gpu_ennaf_opts *opts, int format,
                               uint32_t shard, uint32_t n_shards, naf_gpu_shard_info *info);
size_t naf_gpu_ennaf_shard_bound(size_t slice_len);
/* Step 2.  infos[n_shards] in shard order (this context's own among them).  NAF_GPU_EINPUT + last_error when any shard failed. */
int  naf_gpu_ennaf_shard_finish(naf_gpu_ctx *ctx, const naf_gpu_ennaf_opts *opts, const naf_gpu_shard_info *infos,
                                void *d_pieces, size_t cap, naf_gpu_shard_pieces *pieces);
/* What the finish of shard `shard` applies on behalf of its neighbours, derived from the infos alone (host only, no device needed;
 * exported so that hosts can log it and tests can check it against the reference's chunk-to-chunk state). */
typedef struct {
    uint64_t first_record;      /* records in the shards in front (numbers the reference's messages) */
    uint64_t tail_extra;        /* bases of later shards that belong to this shard's last record */
    uint64_t run_ext;           /* bases of later shards that continue this shard's last soft-mask run */
    uint32_t skip_first;        /* 1: the shard's first base is the high nibble of an earlier shard's last packed byte */
    uint32_t tail_hi;           /* 4-bit code completing the shard's last packed byte when its pack window is odd */
    int32_t  prev_masked;       /* case in front of the shard's first base */
    int32_t  skip_run0;         /* 1: the bases in front of the shard's first case change are emitted by an earlier shard's run */
    uint8_t  first[6], last[6]; /* per stream: this part opens the frame (2-byte header) / closes it (last-block flag) */
    uint8_t  pad_[4];
} naf_gpu_shard_carry;
int  naf_gpu_ennaf_shard_carry(const naf_gpu_shard_info *infos, uint32_t n_shards, uint32_t shard, naf_gpu_shard_carry *out);
/* Step 3 (host only, no device needed).  segs: at least 7 + 6 * n_shards entries; lit: at least 256 + strlen(title) bytes.
 * report (optional) receives the totals of the whole input. */
int  naf_gpu_ennaf_stitch_plan(const naf_gpu_ennaf_opts *opts, const naf_gpu_shard_info *infos, const naf_gpu_shard_pieces *pieces,
                               uint32_t n_shards, naf_gpu_stitch_seg *segs, size_t seg_cap, size_t *n_segs,
                               uint8_t *lit, size_t lit_cap, size_t *lit_len, uint64_t *naf_len, naf_gpu_ennaf_report *report);
/* Execute a plan when this process can address every piece buffer (one device, or peers with access enabled). */
int  naf_gpu_ennaf_stitch(naf_gpu_ctx *ctx, const naf_gpu_stitch_seg *segs, size_t n_segs, const uint8_t *lit,
                          const void *const *d_piece_bufs, void *d_naf, size_t naf_cap);

/* ---- switches ------------------------------------------------------------------------------------------
 * The library's cross-check levers and development aids (INTEGRATION.md section 6 lists them).  naf_gpu_init reads the NAF_GPU_<NAME>
 * variables of the environment ONCE into the context; no later call looks at the environment.  naf_gpu_set_option changes one
 * afterwards (name with or without the NAF_GPU_ prefix; value NULL = not set).  None is needed in production.
 * TRACE=1: the calls keep the verdicts of the paths they took ("[flat mixed] nblk ... decoded ...") as text in the context instead of
 * printing anything; naf_gpu_get_trace returns what has accumulated (valid until the next call on the context), naf_gpu_clear_trace
 * empties it.  The tests ask through this which kernels ran. */
int         naf_gpu_set_option(naf_gpu_ctx *ctx, const char *name, const char *value);
const char *naf_gpu_get_trace(naf_gpu_ctx *ctx);
void        naf_gpu_clear_trace(naf_gpu_ctx *ctx);

/* ---- instrumentation ---------------------------------------------------------------------------------- */
/* Per-kernel device time (hipEvent pairs on the ctx stream) of the last call, for bench.py's roofline
 * object.  names[i] points to static strings.  Returns the number of entries written (<= cap). */
int  naf_gpu_set_timing(naf_gpu_ctx *ctx, int enable);
int  naf_gpu_get_timing(naf_gpu_ctx *ctx, const char **names, float *ms, int *launches, int cap);
/* kernel time of that aggregation per stream: [0] the caller's stream, [1..4] the side chains' (a call is at least the largest) */
int  naf_gpu_get_timing_streams(naf_gpu_ctx *ctx, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif
