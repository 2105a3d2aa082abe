/*
 * naf_oracle.h -- TEST INFRASTRUCTURE ONLY (the "oracle").
 *
 * CPU restatement, in plain C, of the reference ennaf/unnaf hot path (KirillKryukov/naf v1.3.0)
 * and of the zstd frame format it embeds (facebook/zstd, pinned by the reference only in prose at
 * v1.5.0 -- CHANGELOG.md:10; the zstd/ submodule is empty, so the zstd part restates the published
 * format, RFC 8878).  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library.  The product (naf_amd/, libnaf_gpu.so, ennaf/unnaf CLIs) never links or calls it.
 *
 * Parity pinning: tests/test_oracle_*.py check every function here against
 *   (a) the reference's own fixtures (tests/ *.out-ref, NAFv2.pdf VLE table, nucleotide table),
 *   (b) golden vectors produced by the real reference binaries (oracle/_ref, built from
 *       /root/reference by oracle/Makefile) and by the image's libzstd -- tests/golden/.
 */
#ifndef NAF_ORACLE_H
#define NAF_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- zstd (RFC 8878) : zstd_spec.c ------------------------------------------------------- */
/* Decompress ONE zstd frame (with magic).  Returns bytes produced, or <0 on error.
 * *consumed (optional) receives the number of source bytes the frame occupied. */
long long nafo_zstd_decompress_frame(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap,
                                     size_t *consumed);
/* Decompress a concatenation of frames (what one-shot ZSTD_decompress accepts). */
long long nafo_zstd_decompress(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);
/* Content size by walking (decoding) the frame(s); <0 on error. */
long long nafo_zstd_decompressed_size(const uint8_t *src, size_t src_len);
/* Store `src` as one zstd frame of Raw blocks (valid for any conformant decoder).  Returns size. */
long long nafo_zstd_store_raw(const uint8_t *src, size_t src_len, uint8_t *dst, size_t dst_cap);

typedef struct {
    uint32_t n_blocks, n_raw, n_rle, n_compressed;
    uint32_t lit_raw, lit_rle, lit_huf, lit_treeless;
    uint32_t seq_blocks;            /* compressed blocks with nbSeq > 0 */
    uint64_t n_sequences;
    uint32_t mode_count[3][4];      /* [LL,OF,ML][predefined,rle,fse,repeat] */
    uint32_t window_log;            /* 0 when single-segment */
    uint32_t single_segment, has_checksum, has_fcs;
    uint64_t max_offset;
} nafo_zstd_frame_info;
/* Decode the first frame and report its shape (test-side classification of golden frames). */
long long nafo_zstd_frame_info_get(const uint8_t *src, size_t src_len, nafo_zstd_frame_info *info);

/* The blocks and sequences of the first frame as the decoder meets them (tests that plant matches and look for them). */
typedef struct { uint32_t type, size; } nafo_zstd_block;          /* Block_Type 0 Raw, 1 RLE, 2 Compressed; decoded size */
typedef struct {
    uint32_t block;                 /* number of the block that holds the sequence */
    uint32_t offset_value;          /* Offset_Value as coded: 1..3 are repeat codes, else distance + 3 */
    uint64_t pos;                   /* position of the match's first byte in the frame's output */
    uint64_t ll, ml, distance;      /* Literals_Length, Match_Length, the resolved distance */
} nafo_zstd_seq;
typedef struct { nafo_zstd_block *blocks; size_t n_blocks, cap_blocks; nafo_zstd_seq *seqs; size_t n_seqs, cap_seqs; } nafo_zstd_seqlist;
/* Decode the first frame and list it; returns the decoded size or <0 (the list is then empty).  Free with nafo_zstd_seqlist_free. */
long long nafo_zstd_sequences(const uint8_t *src, size_t src_len, nafo_zstd_seqlist *list);
void nafo_zstd_seqlist_free(nafo_zstd_seqlist *list);

/* The literals section of every block of the first frame, as the decoder reads it (tests that hold an encoder's entropy stage to a
 * model).  A Raw or RLE block has lit_type NAFO_LIT_NONE and zeros behind it. */
#define NAFO_LIT_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t block_type, decoded_size, frame_size;   /* Block_Type; bytes the block decodes to; its bytes in the frame, header included */
    uint32_t lit_type;                               /* Literals_Block_Type: 0 Raw, 1 RLE, 2 Compressed (Huffman), 3 Treeless */
    uint32_t regen, comp, header_bytes, n_streams;   /* Regenerated_Size; Compressed_Size (Raw: regen, RLE: 1); 1 to 5; 0 (Raw / RLE), 1 or 4 */
    uint32_t stream_size[4];                         /* one stream: [0] */
    uint32_t tree_bytes, tree_fse, n_weights;        /* the tree description of THIS block (0 bytes: none); FSE-coded or direct; weights written */
    uint32_t n_sequences;
    uint32_t tree_offset;                            /* where this block's tree description begins, from the frame's first byte */
    uint8_t  len[256];                               /* code lengths in force for this block's streams (a treeless block: the inherited ones) */
} nafo_zstd_litblock;
typedef struct { nafo_zstd_litblock *blocks; size_t n, cap; } nafo_zstd_litlist;
long long nafo_zstd_literals(const uint8_t *src, size_t src_len, nafo_zstd_litlist *list);
void nafo_zstd_litlist_free(nafo_zstd_litlist *list);

/* The sequences section of every block of the first frame, as the decoder reads it (tests that hold an encoder's choice of code
 * tables to a model).  Tables are in the order LL, OF, ML.  A block that is not Compressed has zeros behind block_type; a
 * Compressed block without sequences has its one-byte section and zeros behind it. */
typedef struct {
    uint32_t block_type, n_sequences;
    uint32_t nseq_header_bytes;                      /* the Number_of_Sequences field: 1, 2 or 3 */
    uint32_t section_offset, section_bytes;          /* of the Sequences_Section: from the frame's first byte; to the block's end */
    uint32_t bitstream_bytes;
    uint32_t mode[3];                                /* 0 Predefined, 1 RLE, 2 FSE_Compressed, 3 Repeat */
    uint32_t accuracy_log[3];                        /* of the table in force (RLE: 0) */
    uint32_t rle_symbol[3];
    uint32_t desc_bytes[3];                          /* the table's own bytes in this block: 0, 1 (RLE) or its description */
    uint32_t final_state[3];                         /* the states the decoder holds at the block's last sequence */
    uint32_t bits_consumed;                          /* bits the decoder read from the bitstream, the initial states included */
    uint32_t marker_bit;                             /* bit position of the final marker, counted from the bitstream's first bit */
    int16_t  norm[3][64];                            /* probabilities in force: -1 "less than 1", 0 absent (RLE: all 0) */
} nafo_zstd_seqtab;
typedef struct { nafo_zstd_seqtab *blocks; size_t n, cap; } nafo_zstd_tablist;
/* seqs, when not NULL, takes what nafo_zstd_sequences lists, from the same reading.  Unlike the decoders this listing goes on when a
 * bitstream holds bits that no sequence read (bits_consumed < marker_bit): it reports them. */
long long nafo_zstd_seq_tables(const uint8_t *src, size_t src_len, nafo_zstd_tablist *list, nafo_zstd_seqlist *seqs);
void nafo_zstd_tablist_free(nafo_zstd_tablist *list);

/* ---- NAF transforms : naf_oracle.c -------------------------------------------------------- */
enum { NAFO_DNA = 0, NAFO_RNA = 1, NAFO_PROTEIN = 2, NAFO_TEXT = 3 };
enum { NAFO_FMT_UNKNOWN = 0, NAFO_FMT_FASTA = 1, NAFO_FMT_FASTQ = 2 };

typedef struct { uint8_t *data; size_t len, cap; } nafo_buf;

/* Result of the ennaf parse/split stage (reference: ennaf/src/process.c, encoders.c). */
typedef struct {
    int      format;                /* NAFO_FMT_* as sniffed (process.c:547-583) */
    uint64_t n_sequences;
    uint64_t longest_line;
    uint64_t n_bases;               /* seq_size_original */
    nafo_buf ids, comments, lengths, mask, seq, qual;   /* seq = packed 4-bit (DNA/RNA) or text */
    uint64_t unexpected_id[257], unexpected_comment[257], unexpected_seq[257], unexpected_qual[257];
    char     error[256];            /* die() message if the reference would have died */
} nafo_split;

/* Tolerant (default) or --well-formed parser.  Returns 0, or -1 with s->error set (reference die). */
int  nafo_split_text(const uint8_t *text, size_t len, int seq_type, int no_mask, int well_formed,
                     int forced_format, nafo_split *s);
void nafo_split_free(nafo_split *s);

/* Container writer (ennaf.c:538-589).  Each stream is stored as a Raw-block zstd frame.
 * line_length < 0 => use s->longest_line.  Returns bytes written or <0. */
long long nafo_write_naf(const nafo_split *s, int seq_type, int no_mask, long long line_length,
                         const char *title, uint8_t *dst, size_t dst_cap);

/* VLE numbers (encoders.c:175-190, unnaf utils.c:117-141). */
size_t    nafo_vle_write(uint64_t v, uint8_t out[10]);
/* returns bytes consumed, 0 on truncation, -1 on leading 0x80, -2 on overflow */
int       nafo_vle_read(const uint8_t *p, size_t len, uint64_t *v);

typedef struct {
    int      version, seq_type, flags;
    uint8_t  separator;
    uint64_t line_length, n_sequences;
    const uint8_t *title; uint64_t title_len;
    /* per section: original size, compressed size (without magic), pointer to frame[4:] */
    uint64_t orig[6], comp[6]; const uint8_t *payload[6];    /* ids,comments,lengths,mask,seq,qual */
    size_t   header_bytes;
    char     error[128];
} nafo_naf;
enum { NAFO_IDS = 0, NAFO_COMMENTS, NAFO_LENGTHS, NAFO_MASK, NAFO_SEQ, NAFO_QUAL };
int nafo_parse_naf(const uint8_t *naf, size_t len, nafo_naf *h);

/* Whole-file unnaf (unnaf.c:356-456 dispatch; output.c, output-fastq.c).
 * mode: 0 FASTA, 1 FASTQ, 2 --seq, 3 --sequences, 4 --4bit ; -1 = default (FASTQ if quality).
 * line_length_override < 0 => use stored.  Returns bytes written or <0 (h/err in errbuf). */
long long nafo_unnaf(const uint8_t *naf, size_t len, int mode, int use_mask, long long line_length_override,
                     uint8_t *dst, size_t dst_cap, char errbuf[128]);
/* Upper bound of the output size for a mode (exact for FASTA/FASTQ). */
long long nafo_unnaf_size(const uint8_t *naf, size_t len, int mode, long long line_length_override);

/* Building blocks, exported for unit parity tests. */
void   nafo_pack_4bit(const uint8_t *bases, size_t n, uint8_t *out /* (n+1)/2 */);
void   nafo_unpack_4bit(const uint8_t *packed, size_t n_bases, int rna, uint8_t *out);
size_t nafo_mask_rle(const uint8_t *bases, size_t n, uint8_t *units, size_t cap);   /* whole-stream */
void   nafo_mask_apply(uint8_t *bases, size_t n, const uint8_t *units, size_t n_units);

#ifdef __cplusplus
}
#endif
#endif
