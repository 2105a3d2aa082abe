"""ctypes binding of the libnaf_gpu.so C-ABI (include/naf_gpu.h).

Used by the tests and bench.py; the shipped hosts are the C programs in naf_amd/host/.  Device
buffers are torch uint8 CUDA(HIP) tensors -- torch is plumbing for HBM allocations and streams only.
There is no CPU fallback: loading fails loudly if the shared library is missing, and `Context()`
raises if no gfx950 device is usable.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NAF_GPU_LIB") or os.path.join(_HERE, "libnaf_gpu.so")       # NAF_GPU_LIB: another build of the same C-ABI (A / B measurements)

OUT_DEFAULT, OUT_FASTA, OUT_FASTQ, OUT_SEQ, OUT_SEQUENCES, OUT_4BIT = -1, 0, 1, 2, 3, 4
SEQ_DNA, SEQ_RNA, SEQ_PROTEIN, SEQ_TEXT = 0, 1, 2, 3
FMT_AUTO, FMT_FASTA, FMT_FASTQ = 0, 1, 2
E_CAP = -6

EXPORTS = [
    "naf_gpu_init", "naf_gpu_shutdown", "naf_gpu_strerror", "naf_gpu_last_error", "naf_gpu_set_stream",
    "naf_gpu_synchronize", "naf_gpu_reserve", "naf_gpu_malloc", "naf_gpu_free", "naf_gpu_host_alloc",
    "naf_gpu_host_free", "naf_gpu_upload", "naf_gpu_download", "naf_gpu_download_async", "naf_gpu_histogram", "naf_gpu_zstd_decompress",
    "naf_gpu_mem_info", "naf_gpu_release_scratch", "naf_gpu_zstd_compress", "naf_gpu_zstd_compress_bound", "naf_gpu_parse_header", "naf_gpu_parse_header_host",
    "naf_gpu_unnaf_size", "naf_gpu_unnaf", "naf_gpu_unnaf_range", "naf_gpu_ennaf_bound", "naf_gpu_ennaf",
    "naf_gpu_set_timing", "naf_gpu_get_timing",
    "naf_gpu_ennaf_sniff", "naf_gpu_ennaf_count_lines", "naf_gpu_ennaf_find_cut", "naf_gpu_ennaf_shard_begin", "naf_gpu_ennaf_shard_bound",
    "naf_gpu_ennaf_shard_finish", "naf_gpu_ennaf_shard_carry", "naf_gpu_ennaf_stitch_plan", "naf_gpu_ennaf_stitch",
    "naf_gpu_read_file", "naf_gpu_write_file", "naf_gpu_copy", "naf_gpu_gather_ranges", "naf_gpu_get_timing_streams",
    "naf_gpu_set_option", "naf_gpu_get_trace", "naf_gpu_clear_trace", "naf_gpu_write_fd",
    "naf_gpu_unnaf_find", "naf_gpu_unnaf_record_table", "naf_gpu_unnaf_select_size", "naf_gpu_unnaf_select", "naf_gpu_parse_region",
    "naf_gpu_unnaf_select_stranded_size", "naf_gpu_unnaf_select_stranded",
    "naf_gpu_compile_motif", "naf_gpu_unnaf_locate_count", "naf_gpu_unnaf_locate",
    "naf_gpu_compile_motif_near", "naf_gpu_unnaf_locate_near_count", "naf_gpu_unnaf_locate_near",
    "naf_gpu_composition_rows_of", "naf_gpu_unnaf_composition_rows", "naf_gpu_unnaf_composition",
    "naf_gpu_quality_error_table", "naf_gpu_unnaf_quality_rows", "naf_gpu_unnaf_quality",
    "naf_gpu_parse_base_class", "naf_gpu_unnaf_runs_count", "naf_gpu_unnaf_runs",
    "naf_gpu_kmer_index", "naf_gpu_kmer_text", "naf_gpu_unnaf_kmers_rows", "naf_gpu_unnaf_kmers",
    "naf_gpu_parse_codon_set", "naf_gpu_unnaf_orfs_count", "naf_gpu_unnaf_orfs",
    "naf_gpu_genetic_code_by_id", "naf_gpu_genetic_code_parse", "naf_gpu_genetic_code_stops", "naf_gpu_codon_lut",
    "naf_gpu_unnaf_translate_size", "naf_gpu_unnaf_translate",
    "naf_gpu_parse_repeat_spec", "naf_gpu_repeat_class", "naf_gpu_unnaf_repeats_count", "naf_gpu_unnaf_repeats",
    "naf_gpu_trim_limit", "naf_gpu_unnaf_trim", "naf_gpu_unnaf_select_reads_size", "naf_gpu_unnaf_select_reads",
    "naf_gpu_clip_budgets", "naf_gpu_unnaf_clip",
    "naf_gpu_dedup_level", "naf_gpu_unnaf_dedup",
    "naf_gpu_unnaf_screen",
]
WHOLE = 2 ** 64 - 1                     # NAF_GPU_WHOLE: (record, 0, WHOLE) is the record as stored
MAX_SHARDS = 64


class UnnafOpts(C.Structure):
    _fields_ = [("out_type", C.c_int), ("use_mask", C.c_int), ("line_length", C.c_int64)]


class Header(C.Structure):
    _fields_ = [("version", C.c_int), ("seq_type", C.c_int), ("flags", C.c_int), ("separator", C.c_uint8),
                ("line_length", C.c_uint64), ("n_sequences", C.c_uint64), ("title_off", C.c_uint64), ("title_len", C.c_uint64),
                ("orig_size", C.c_uint64 * 6), ("comp_size", C.c_uint64 * 6), ("payload_off", C.c_uint64 * 6)]


class EnnafOpts(C.Structure):
    _fields_ = [("format", C.c_int), ("seq_type", C.c_int), ("no_mask", C.c_int), ("strict", C.c_int), ("level", C.c_int),
                ("line_length", C.c_int64), ("title", C.c_char_p), ("long_log", C.c_int)]


class EnnafReport(C.Structure):
    _fields_ = [("format", C.c_int), ("n_sequences", C.c_uint64), ("n_bases", C.c_uint64), ("longest_line", C.c_uint64),
                ("unexpected_id", C.c_uint64 * 257), ("unexpected_comment", C.c_uint64 * 257),
                ("unexpected_seq", C.c_uint64 * 257), ("unexpected_qual", C.c_uint64 * 257),
                ("section_orig", C.c_uint64 * 6), ("section_comp", C.c_uint64 * 6)]


class ShardInfo(C.Structure):
    """naf_gpu_shard_info: what one shard of a multi-GPU ennaf tells the others (exchanged verbatim as bytes)."""
    _fields_ = [("shard", C.c_uint32), ("n_shards", C.c_uint32), ("format", C.c_int32), ("seq_type", C.c_int32), ("text_len", C.c_uint64),
                ("n_sequences", C.c_uint64), ("n_bases", C.c_uint64), ("longest_line", C.c_uint64), ("lead_bases", C.c_uint64),
                ("n_ids", C.c_uint64), ("n_comments", C.c_uint64), ("n_quality", C.c_uint64),
                ("mask_changes", C.c_uint64), ("mask_first_change", C.c_uint64), ("mask_last_change", C.c_uint64),
                ("first_base", C.c_uint8), ("last_base", C.c_uint8), ("store_mask", C.c_uint8), ("store_quality", C.c_uint8), ("pad_", C.c_uint8 * 4),
                ("err_kind", C.c_int32), ("err_char", C.c_uint32), ("err_record", C.c_uint64), ("err_a", C.c_uint64), ("err_b", C.c_uint64),
                ("unexpected", (C.c_uint64 * 257) * 4)]


class ShardPieces(C.Structure):
    _fields_ = [("off", C.c_uint64 * 6), ("len", C.c_uint64 * 6), ("raw", C.c_uint64 * 6), ("total", C.c_uint64)]


class ShardCarry(C.Structure):
    _fields_ = [("first_record", C.c_uint64), ("tail_extra", C.c_uint64), ("run_ext", C.c_uint64), ("skip_first", C.c_uint32), ("tail_hi", C.c_uint32),
                ("prev_masked", C.c_int32), ("skip_run0", C.c_int32), ("first", C.c_uint8 * 6), ("last", C.c_uint8 * 6), ("pad_", C.c_uint8 * 4)]


class StitchSeg(C.Structure):
    _fields_ = [("dst_off", C.c_uint64), ("len", C.c_uint64), ("src_off", C.c_uint64), ("shard", C.c_int32), ("stream", C.c_int32)]


class Segment(C.Structure):
    """naf_gpu_segment: bases [begin, end) of a record, 0-based."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64)]


class GeneticCode(C.Structure):
    """naf_gpu_genetic_code: aa[i] is the letter of the codon of index i under kmer_index at K = 3 (AAA AAC AAG AAT ACA ...); '*' = stop."""
    _fields_ = [("aa", C.c_char * 64)]

    @property
    def letters(self):
        return bytes(self.aa).decode("latin1")


class Hit(C.Structure):
    """naf_gpu_hit: pattern number `pattern` matches at bases [begin, begin + its length) of `record`; strand 1 = the reverse complement
    of those bases does."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("pattern", C.c_uint32), ("strand", C.c_uint32)]


HIT_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("pattern", "<u4"), ("strand", "<u4")]      # numpy's view of a table of hits
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 1, 2, 3


class NearHit(C.Structure):
    """naf_gpu_near_hit: pattern number `pattern` lies at bases [begin, begin + its length) of `record` with `mismatches` letters that
    do not match; `where` has bit j set when letter j of the pattern as written (brackets not counted) is one of them."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("pattern", C.c_uint32), ("strand", C.c_uint32), ("mismatches", C.c_uint32), ("where", C.c_uint32)]


NEAR_HIT_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("pattern", "<u4"), ("strand", "<u4"), ("mismatches", "<u4"), ("where", "<u4")]      # numpy's view of a table of near hits
NEAR_HIT_BYTES = 32
LOCATE_MAX_MISMATCHES = 8


class CompRow(C.Structure):
    """naf_gpu_comp_row: the composition of bases [begin, end) of `record`: n[c] bases of 4-bit code c ("-TGKCYSBAWRDMHVN"), the
    soft-masked ones, and the C's that a G of the same record follows."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("n", C.c_uint64 * 16), ("masked", C.c_uint64), ("cpg", C.c_uint64)]


COMP_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("n", "<u8", (16,)), ("masked", "<u8"), ("cpg", "<u8")]      # numpy's view of a table of rows
COMP_ROW_BYTES = 168
COMP_MASK = 1


class QualRow(C.Structure):
    """naf_gpu_qual_row: the quality codes of one read (key: its number) or of one bin of read positions (key: the bin's number): how
    many, the sum of their bytes, the sum of their error-table entries (expected errors times 2^32), those at or above Q20 and Q30
    (Phred+33), and the smallest and largest byte (255 and 0 in a row without codes)."""
    _fields_ = [("key", C.c_uint64), ("n", C.c_uint64), ("sum", C.c_uint64), ("ee", C.c_uint64), ("n_q20", C.c_uint64), ("n_q30", C.c_uint64),
                ("min", C.c_uint32), ("max", C.c_uint32)]


QUAL_DTYPE = [("key", "<u8"), ("n", "<u8"), ("sum", "<u8"), ("ee", "<u8"), ("n_q20", "<u8"), ("n_q30", "<u8"), ("min", "<u4"), ("max", "<u4")]      # numpy's view of a table of rows
QUAL_ROW_BYTES = 56


class Run(C.Structure):
    """naf_gpu_run: bases [begin, end) of `record` are a run -- of a base class (code: the 4-bit code of its first base; with RUNS_EACH
    the code of all of them) or of soft-masked bases (code 0)."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("code", C.c_uint32), ("reserved", C.c_uint32)]


RUN_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("code", "<u4"), ("reserved", "<u4")]      # numpy's view of a table of runs
RUN_BYTES = 32
RUNS_EACH, RUNS_MASKED = 1, 2


class KmerRow(C.Structure):
    """naf_gpu_kmer_row: the k-mers of one record (begin 0, end its length) or, as a total, of `record` records with `end` bases:
    `positions` start positions that have K bases in their record, `counted` of them whose K bases are all stored as A, C, G or T/U."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("positions", C.c_uint64), ("counted", C.c_uint64)]


KMER_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("positions", "<u8"), ("counted", "<u8")]      # numpy's view of a table of rows
KMER_ROW_BYTES = 40
KMER_CANONICAL, KMER_PER_RECORD = 1, 2
KMER_MAX_K = 12


class Orf(C.Structure):
    """naf_gpu_orf: bases [begin, end) of `record` (forward offsets, the stop codon not included) are an open reading frame of strand 0
    (as stored) or 1 (the reverse complement), frame 0..2 (reverse: counted from the record's end); flags: ORF_STOP3, ORF_STOP5."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("strand", C.c_uint32), ("frame", C.c_uint16), ("flags", C.c_uint16)]


ORF_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("strand", "<u4"), ("frame", "<u2"), ("flags", "<u2")]      # numpy's view of a table of ORFs
ORF_BYTES = 32
ORF_STOP3, ORF_STOP5 = 1, 2                   # a row's flags
ORF_SPLIT_UNKNOWN, ORF_CLOSED = 1, 2          # a call's flags


class Repeat(C.Structure):
    """naf_gpu_repeat: bases [begin, end) of `record` are a tandem repeat of `period` bases; motif: its first `period` bases, base i at bits
    2i and 2i + 1 (A 0, C 1, G 2, T/U 3)."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("motif", C.c_uint32), ("period", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class RepeatSpec(C.Structure):
    """naf_gpu_repeat_spec: min_copies[p - 1] = the copies a repeat of period p needs (>= 2), 0: the period is not searched."""
    _fields_ = [("min_copies", C.c_uint32 * 16)]


# numpy's view of a table of tandem repeats (naf_gpu_repeat): bases [begin, end) of `record` repeat the `period` bases of `motif` (base i at
# bits 2i, 2i + 1: A 0, C 1, G 2, T/U 3)
REPEAT_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("motif", "<u4"), ("period", "u1"), ("reserved", "u1", (3,))]
REPEAT_BYTES = 32
REPEATS_WHOLE_UNITS = 1


class TrimOpts(C.Structure):
    """naf_gpu_trim_opts: the cutoff error rate times 2^32 (TRIM_NONE: no trimming), the bases a kept read needs, the expected errors times
    2^32 it may have (2^64 - 1: any)."""
    _fields_ = [("limit", C.c_uint64), ("min_len", C.c_uint64), ("max_ee", C.c_uint64)]


class TrimRow(C.Structure):
    """naf_gpu_trim_row: bases [begin, end) of `record` are the stretch to keep, ee the sum of the error-table entries of its quality codes;
    flags: TRIM_KEPT, or TRIM_SHORT and / or TRIM_ERRORS."""
    _fields_ = [("record", C.c_uint64), ("begin", C.c_uint64), ("end", C.c_uint64), ("ee", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TrimTotal(C.Structure):
    """naf_gpu_trim_total: the reads of a call, those kept, all their bases, the bases and the ee of the kept stretches, the rows with
    TRIM_SHORT and with TRIM_ERRORS."""
    _fields_ = [("reads", C.c_uint64), ("kept", C.c_uint64), ("bases", C.c_uint64), ("kept_bases", C.c_uint64), ("kept_ee", C.c_uint64),
                ("n_short", C.c_uint64), ("n_errors", C.c_uint64)]


TRIM_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("ee", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]      # numpy's view of a table of rows
TRIM_BYTES = 40
TRIM_KEPT, TRIM_SHORT, TRIM_ERRORS = 1, 2, 4
TRIM_NONE = 2 ** 64 - 1


class ClipOpts(C.Structure):
    """naf_gpu_clip_opts: the letters of an adapter that must overlap the read, the bases a kept read needs."""
    _fields_ = [("min_overlap", C.c_uint32), ("min_len", C.c_uint64)]


class ClipTotal(C.Structure):
    """naf_gpu_clip_total: the reads of a call, those an adapter was found in, those kept, the bases of their windows, the bases of the kept
    stretches, the bases behind the clip points, the rows with TRIM_SHORT and with TRIM_ERRORS."""
    _fields_ = [("reads", C.c_uint64), ("clipped", C.c_uint64), ("kept", C.c_uint64), ("bases", C.c_uint64), ("kept_bases", C.c_uint64),
                ("removed_bases", C.c_uint64), ("n_short", C.c_uint64), ("n_errors", C.c_uint64)]


# numpy's view of a table of naf_gpu_clip_row: bases [begin, end) of `record` are kept; adapter: the number of the adapter that begins at
# `end` (CLIP_NO_ADAPTER: none) with `mismatches` among the `overlap` letters of it the window holds; flags: TRIM_KEPT, or TRIM_SHORT and /
# or TRIM_ERRORS, and CLIP_CLIPPED
CLIP_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("adapter", "<u4"), ("mismatches", "<u4"), ("overlap", "<u4"), ("flags", "<u4")]
CLIP_BYTES = 40
CLIP_CLIPPED = 8
CLIP_NO_ADAPTER = 2 ** 32 - 1
CLIP_MAX_ADAPTERS = 16


class DedupOpts(C.Structure):
    """naf_gpu_dedup_opts: DEDUP_BOTH_STRANDS or 0; which call wrote the bounds rows (DEDUP_BOUNDS_TRIM, DEDUP_BOUNDS_CLIP)."""
    _fields_ = [("flags", C.c_uint32), ("bounds_kind", C.c_uint32)]


class DedupTotal(C.Structure):
    """naf_gpu_dedup_total: the reads of a call, those that take part, their classes, the copies among them, the classes of one, the largest
    class, the bases of the windows that take part and of the firsts' windows."""
    _fields_ = [("reads", C.c_uint64), ("considered", C.c_uint64), ("classes", C.c_uint64), ("duplicates", C.c_uint64), ("singletons", C.c_uint64),
                ("largest", C.c_uint64), ("bases", C.c_uint64), ("kept_bases", C.c_uint64)]


# numpy's view of a table of naf_gpu_dedup_row: bases [begin, end) of `record` are its window; first: the smallest record of its class;
# copies: the records in the class; flags: TRIM_KEPT (the class's first) or DEDUP_DUPLICATE, and CLIP_CLIPPED carried -- of a record that
# takes no part the bounds row's flags; strand: 1 when the window equals only the reverse complement of the first's
DEDUP_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("first", "<u8"), ("copies", "<u8"), ("flags", "<u4"), ("strand", "<u4")]
DEDUP_BYTES = 48
DEDUP_DUPLICATE = 16
DEDUP_BOTH_STRANDS = 1
DEDUP_BOUNDS_TRIM, DEDUP_BOUNDS_CLIP = 0, 1
DEDUP_LEVELS = 16


class ScreenOpts(C.Structure):
    """naf_gpu_screen_opts: K (1 to 31); SCREEN_KEEP_MATCHED | SCREEN_FORWARD_ONLY or 0; which call wrote the bounds rows (SCREEN_BOUNDS_TRIM,
    _CLIP, _DEDUP); the hits that make a read matched (1 or more)."""
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("bounds_kind", C.c_uint32), ("min_hits", C.c_uint64)]


class ScreenTotal(C.Structure):
    """naf_gpu_screen_total: the reads of a call, those that take part, those matched, those kept, the bases of the windows that take part
    and of the kept ones, the valid k-mer positions in those windows and the ones that hit; the reference's records, bases, valid positions
    and distinct keys."""
    _fields_ = [("reads", C.c_uint64), ("considered", C.c_uint64), ("matched", C.c_uint64), ("kept", C.c_uint64), ("bases", C.c_uint64),
                ("kept_bases", C.c_uint64), ("kmers", C.c_uint64), ("hit_kmers", C.c_uint64), ("ref_records", C.c_uint64), ("ref_bases", C.c_uint64),
                ("ref_positions", C.c_uint64), ("ref_kmers", C.c_uint64)]


# numpy's view of a table of naf_gpu_screen_row: bases [begin, end) of `record` are its window, `hits` of its k-mers are in the reference's
# set; flags: SCREEN_MATCHED, TRIM_KEPT (kept under the verdict) and CLIP_CLIPPED carried -- of a record that takes no part the bounds
# row's flags.  A trim row with hits where ee stands: unnaf_dedup takes the table as bounds_kind "trim".
SCREEN_DTYPE = [("record", "<u8"), ("begin", "<u8"), ("end", "<u8"), ("hits", "<u8"), ("flags", "<u4"), ("reserved", "<u4")]
SCREEN_BYTES = 40
SCREEN_MATCHED = 32
SCREEN_KEEP_MATCHED, SCREEN_FORWARD_ONLY = 1, 2
SCREEN_BOUNDS_TRIM, SCREEN_BOUNDS_CLIP, SCREEN_BOUNDS_DEDUP = 0, 1, 2
SCREEN_MAX_K = 31


class NafGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("naf_gpu error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


_lib = None


def load():
    """dlopen libnaf_gpu.so (no HIP call is made here, so this works on a machine without a GPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libnaf_gpu.so is not built (run `make` or __graft_entry__.build()); there is no CPU fallback")
        # torch first, when it is there: it brings its own libamdhip64, and the library must bind to the HIP runtime the process
        # already has -- loaded the other way round (library, then torch) the process holds two runtimes and naf_gpu_init finds no
        # device.  The C hosts link /opt/rocm's runtime and never see torch.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
        L.naf_gpu_init.argtypes = [i, C.POINTER(vp)]
        L.naf_gpu_shutdown.argtypes = [vp]
        L.naf_gpu_shutdown.restype = None
        L.naf_gpu_strerror.restype = C.c_char_p
        L.naf_gpu_last_error.restype = C.c_char_p
        L.naf_gpu_last_error.argtypes = [vp]
        L.naf_gpu_set_stream.argtypes = [vp, vp]
        L.naf_gpu_synchronize.argtypes = [vp]
        L.naf_gpu_reserve.argtypes = [vp, sz]
        L.naf_gpu_histogram.argtypes = [vp, vp, sz, C.POINTER(C.c_uint64)]
        L.naf_gpu_zstd_decompress.argtypes = [vp, vp, sz, i, vp, sz, C.POINTER(sz)]
        L.naf_gpu_parse_header.argtypes = [vp, vp, sz, C.POINTER(Header)]
        L.naf_gpu_parse_header_host.argtypes = [C.c_char_p, sz, C.POINTER(Header), C.c_char_p]
        L.naf_gpu_unnaf_size.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(sz)]
        L.naf_gpu_unnaf.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), vp, sz, C.POINTER(sz)]
        L.naf_gpu_unnaf_range.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.c_uint64, C.c_uint64, vp, sz, C.POINTER(sz)]
        L.naf_gpu_set_timing.argtypes = [vp, i]
        L.naf_gpu_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(i), i]
        for opt in ("naf_gpu_zstd_compress", "naf_gpu_ennaf"):
            if hasattr(L, opt):
                pass
        if hasattr(L, "naf_gpu_zstd_compress"):
            L.naf_gpu_zstd_compress.argtypes = [vp, vp, sz, i, vp, sz, C.POINTER(sz)]
            L.naf_gpu_zstd_compress_bound.argtypes = [sz]
            L.naf_gpu_zstd_compress_bound.restype = sz
        if hasattr(L, "naf_gpu_ennaf"):
            L.naf_gpu_ennaf.argtypes = [vp, vp, sz, C.POINTER(EnnafOpts), vp, sz, C.POINTER(sz), C.POINTER(EnnafReport)]
            L.naf_gpu_ennaf_bound.argtypes = [sz]
            L.naf_gpu_ennaf_bound.restype = sz
        u64p = C.POINTER(C.c_uint64)
        L.naf_gpu_ennaf_sniff.argtypes = [vp, vp, sz, i, C.POINTER(i), u64p]
        L.naf_gpu_ennaf_count_lines.argtypes = [vp, vp, sz, i, u64p]
        L.naf_gpu_ennaf_find_cut.argtypes = [vp, vp, sz, i, i, C.c_uint64, u64p]
        L.naf_gpu_ennaf_shard_begin.argtypes = [vp, vp, sz, C.POINTER(EnnafOpts), i, C.c_uint32, C.c_uint32, C.POINTER(ShardInfo)]
        L.naf_gpu_ennaf_shard_bound.argtypes = [sz]
        L.naf_gpu_ennaf_shard_bound.restype = sz
        L.naf_gpu_ennaf_shard_finish.argtypes = [vp, C.POINTER(EnnafOpts), C.POINTER(ShardInfo), vp, sz, C.POINTER(ShardPieces)]
        L.naf_gpu_ennaf_shard_carry.argtypes = [C.POINTER(ShardInfo), C.c_uint32, C.c_uint32, C.POINTER(ShardCarry)]
        L.naf_gpu_ennaf_stitch_plan.argtypes = [C.POINTER(EnnafOpts), C.POINTER(ShardInfo), C.POINTER(ShardPieces), C.c_uint32, C.POINTER(StitchSeg), sz,
                                                C.POINTER(sz), C.c_char_p, sz, C.POINTER(sz), u64p, C.POINTER(EnnafReport)]
        L.naf_gpu_ennaf_stitch.argtypes = [vp, C.POINTER(StitchSeg), sz, C.c_char_p, C.POINTER(vp), vp, sz]
        L.naf_gpu_copy.argtypes = [vp, vp, vp, sz]
        L.naf_gpu_write_file.argtypes = [vp, i, C.c_uint64, vp, sz]
        L.naf_gpu_read_file.argtypes = [vp, i, C.c_uint64, sz, vp]
        L.naf_gpu_write_fd.argtypes = [vp, i, vp, sz]
        L.naf_gpu_release_scratch.argtypes = [vp]
        L.naf_gpu_mem_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
        L.naf_gpu_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
        L.naf_gpu_host_free.argtypes = [vp, vp]
        L.naf_gpu_upload.argtypes = [vp, vp, vp, sz]
        L.naf_gpu_download.argtypes = [vp, vp, vp, sz]
        L.naf_gpu_download_async.argtypes = [vp, vp, vp, sz]
        L.naf_gpu_get_timing_streams.argtypes = [vp, C.POINTER(C.c_float)]
        L.naf_gpu_gather_ranges.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(vp), u64p, C.POINTER(sz), i]
        L.naf_gpu_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.naf_gpu_get_trace.argtypes = [vp]
        L.naf_gpu_get_trace.restype = C.c_char_p
        L.naf_gpu_clear_trace.argtypes = [vp]
        L.naf_gpu_clear_trace.restype = None
        L.naf_gpu_unnaf_find.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, u64p]
        L.naf_gpu_unnaf_record_table.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_unnaf_select_size.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), sz, C.POINTER(sz)]
        L.naf_gpu_unnaf_select.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), sz, vp, sz, C.POINTER(sz)]
        L.naf_gpu_parse_region.argtypes = [C.c_char_p, C.POINTER(sz), u64p, u64p]
        u8p = C.POINTER(C.c_uint8)
        L.naf_gpu_unnaf_select_stranded_size.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), u8p, sz, C.POINTER(sz)]
        L.naf_gpu_unnaf_select_stranded.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), u8p, sz, vp, sz, C.POINTER(sz)]
        L.naf_gpu_compile_motif.argtypes = [C.c_char_p, u8p, u8p, C.POINTER(sz)]
        L.naf_gpu_unnaf_locate_count.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, i, C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_unnaf_locate.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, i, C.c_uint64, C.c_uint64, vp, sz, u64p]
        u32p = C.POINTER(C.c_uint32)
        L.naf_gpu_compile_motif_near.argtypes = [C.c_char_p, u8p, u8p, u32p, C.POINTER(sz)]
        L.naf_gpu_unnaf_locate_near_count.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, u32p, i, C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_unnaf_locate_near.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, u32p, i, C.c_uint64, C.c_uint64, vp, sz, u64p]
        L.naf_gpu_composition_rows_of.argtypes = [C.c_uint64, C.c_uint64]
        L.naf_gpu_composition_rows_of.restype = C.c_uint64
        L.naf_gpu_unnaf_composition_rows.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
        L.naf_gpu_unnaf_composition.argtypes = [vp, vp, sz, C.c_uint64, i, C.c_uint64, C.c_uint64, vp, sz, u64p, C.POINTER(CompRow)]
        L.naf_gpu_quality_error_table.argtypes = [u64p]
        L.naf_gpu_unnaf_quality_rows.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_unnaf_quality.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, vp, sz, vp, sz, u64p, u64p, u64p, C.POINTER(QualRow)]
        L.naf_gpu_parse_base_class.argtypes = [C.c_char_p, C.POINTER(C.c_uint16)]
        L.naf_gpu_unnaf_runs_count.argtypes = [vp, vp, sz, C.c_uint16, i, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_unnaf_runs.argtypes = [vp, vp, sz, C.c_uint16, i, C.c_uint64, C.c_uint64, C.c_uint64, vp, sz, u64p, u64p]
        L.naf_gpu_kmer_index.argtypes = [C.c_char_p, i, C.POINTER(C.c_uint), u64p]
        L.naf_gpu_kmer_text.argtypes = [C.c_uint, C.c_uint64, C.c_char_p]
        L.naf_gpu_unnaf_kmers_rows.argtypes = [vp, vp, sz, C.c_uint, i, C.c_uint64, C.c_uint64, u64p, u64p]
        L.naf_gpu_parse_codon_set.argtypes = [C.c_char_p, u64p]
        L.naf_gpu_unnaf_orfs_count.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, i, i, C.c_uint64, C.c_uint64, u64p, u64p, u64p]
        L.naf_gpu_unnaf_orfs.argtypes = [vp, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, i, i, C.c_uint64, C.c_uint64, vp, sz, u64p, u64p]
        L.naf_gpu_unnaf_kmers.argtypes = [vp, vp, sz, C.c_uint, i, C.c_uint64, C.c_uint64, vp, sz, vp, sz, u64p, u64p, C.POINTER(KmerRow)]
        L.naf_gpu_genetic_code_by_id.argtypes = [i, C.POINTER(GeneticCode)]
        L.naf_gpu_genetic_code_parse.argtypes = [C.c_char_p, C.POINTER(GeneticCode)]
        L.naf_gpu_genetic_code_stops.argtypes = [C.POINTER(GeneticCode), u64p]
        L.naf_gpu_codon_lut.argtypes = [C.POINTER(GeneticCode), u8p]
        L.naf_gpu_unnaf_translate_size.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(GeneticCode), C.POINTER(Segment), u8p, sz, C.POINTER(sz)]
        L.naf_gpu_unnaf_translate.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(GeneticCode), C.POINTER(Segment), u8p, sz, vp, sz, C.POINTER(sz)]
        L.naf_gpu_parse_repeat_spec.argtypes = [C.c_char_p, C.POINTER(RepeatSpec)]
        L.naf_gpu_repeat_class.argtypes = [C.c_uint32, C.c_uint, u32p]
        L.naf_gpu_unnaf_repeats_count.argtypes = [vp, vp, sz, C.POINTER(RepeatSpec), i, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, u64p]
        L.naf_gpu_unnaf_repeats.argtypes = [vp, vp, sz, C.POINTER(RepeatSpec), i, C.c_uint64, C.c_uint64, C.c_uint64, vp, sz, u64p, u64p, u64p]
        L.naf_gpu_trim_limit.argtypes = [C.c_uint, u64p]
        L.naf_gpu_unnaf_trim.argtypes = [vp, vp, sz, C.POINTER(TrimOpts), C.c_uint64, C.c_uint64, vp, sz, u64p, C.POINTER(TrimTotal)]
        L.naf_gpu_clip_budgets.argtypes = [C.c_uint64, C.c_uint64, C.c_uint, u8p]
        L.naf_gpu_unnaf_clip.argtypes = [vp, vp, sz, C.c_char_p, sz, sz, u8p, C.POINTER(ClipOpts), C.c_uint64, C.c_uint64, vp, vp, sz, u64p, C.POINTER(ClipTotal), u64p]
        L.naf_gpu_dedup_level.argtypes = [C.c_uint64, C.POINTER(C.c_uint)]
        L.naf_gpu_unnaf_dedup.argtypes = [vp, vp, sz, C.POINTER(DedupOpts), C.c_uint64, C.c_uint64, vp, vp, sz, u64p, C.POINTER(DedupTotal), u64p]
        L.naf_gpu_unnaf_screen.argtypes = [vp, vp, sz, vp, sz, C.POINTER(ScreenOpts), C.c_uint64, C.c_uint64, vp, vp, sz, u64p, C.POINTER(ScreenTotal)]
        L.naf_gpu_unnaf_select_reads_size.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), u8p, sz, C.POINTER(sz)]
        L.naf_gpu_unnaf_select_reads.argtypes = [vp, vp, sz, C.POINTER(UnnafOpts), C.POINTER(Segment), u8p, sz, vp, sz, C.POINTER(sz)]
        _lib = L
    return _lib


def _text_arg(text, what):
    """The bytes of a text argument of a host-only parser (str: as latin1); one with a zero byte, where the C side would see the text
    end, is ValueError("not WHAT: ...") like any other text the parser refuses."""
    b = text.encode("latin1") if isinstance(text, str) else bytes(text)
    if b"\0" in b:
        raise ValueError("not %s: %r" % (what, text))
    return b


def parse_region(text):
    """Host-only: "ID", "ID:a-b", "ID:a-", "ID:a" (1-based, inclusive) -> (id, begin, end), 0-based half-open; a whole record is
    (id, 0, WHOLE).  ValueError when the text is no region (naf_gpu_parse_region)."""
    b = text.encode("latin1") if isinstance(text, str) else bytes(text)
    n, lo, hi = C.c_size_t(), C.c_uint64(), C.c_uint64()
    if load().naf_gpu_parse_region(b, C.byref(n), C.byref(lo), C.byref(hi)):
        raise ValueError("not a region: %r" % (text,))
    rid = b[:n.value]
    return (rid.decode("latin1") if isinstance(text, str) else rid), lo.value, hi.value


def compile_motif(text):
    """Host-only: (fwd, rev) -- the 4-bit sets of an IUPAC pattern and of its reverse complement, as bytes of the pattern's length
    (naf_gpu_compile_motif).  ValueError for what is no pattern."""
    b = _text_arg(text, "a pattern")
    fwd, rev, n = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), C.c_size_t()
    if load().naf_gpu_compile_motif(b, fwd, rev, C.byref(n)):
        raise ValueError("not a pattern: %r" % (text,))
    return bytes(fwd[:n.value]), bytes(rev[:n.value])


def compile_motif_near(text):
    """Host-only: (fwd, rev, fixed) of an IUPAC pattern that may hold bracketed runs of must-match letters (naf_gpu_compile_motif_near):
    the 4-bit sets as compile_motif gives them, and the bit mask of the bracketed letters by their index in the pattern, brackets not
    counted.  ValueError for what is no pattern."""
    b = _text_arg(text, "a pattern")
    fwd, rev, fixed, n = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), C.c_uint32(), C.c_size_t()
    if load().naf_gpu_compile_motif_near(b, fwd, rev, C.byref(fixed), C.byref(n)):
        raise ValueError("not a pattern: %r" % (text,))
    return bytes(fwd[:n.value]), bytes(rev[:n.value]), fixed.value


def motif_letters(pattern):
    """A pattern's letters without the brackets of must-match runs (str or bytes, as given)."""
    return pattern.replace("[", "").replace("]", "") if isinstance(pattern, str) else bytes(pattern).replace(b"[", b"").replace(b"]", b"")


def composition_rows_of(n, window):
    """Host-only: the rows a record of n bases gives under `window` (naf_gpu_composition_rows_of): 1 for window 0, else ceil(n / window)."""
    return int(load().naf_gpu_composition_rows_of(int(n), int(window)))


def quality_error_table():
    """Host-only: the 256 entries of naf_gpu_quality_error_table -- the error probability of Phred+33 byte b times 2^32, rounded half up
    (2^32 below 33) -- as a list of ints."""
    tab = (C.c_uint64 * 256)()
    rc = load().naf_gpu_quality_error_table(tab)
    if rc:
        raise NafGpuError(rc, load().naf_gpu_strerror(rc).decode())
    return [int(v) for v in tab]


def trim_limit(q):
    """Host-only: the limit of "trim below Phred q" (naf_gpu_trim_limit): the error-table entry of byte 33 + q, q = 0 .. 93."""
    v = C.c_uint64()
    rc = load().naf_gpu_trim_limit(int(q), C.byref(v)) if 0 <= int(q) < 2 ** 32 else -8
    if rc:
        raise ValueError("not a Phred score to trim at (0 to 93): %r" % (q,))
    return int(v.value)


def _decimal(x, what, plural):
    """A number given as an int, a Fraction, or a decimal text of digits with at most one point that has 1 to 9 digits behind it, as a
    Fraction.  No floats: a float is not the number that was written."""
    from fractions import Fraction
    if isinstance(x, bool) or isinstance(x, float):
        raise ValueError("%s given as text, int or Fraction, not as %r" % (plural, x))
    if isinstance(x, (bytes, str)):
        t = x.decode("latin1") if isinstance(x, bytes) else x
        whole, point, frac = t.partition(".")
        if not (whole.isascii() and whole.isdigit() and ((not point) or (frac.isascii() and frac.isdigit() and 1 <= len(frac) <= 9))):
            raise ValueError("not %s (digits, or digits.digits with 1 to 9 behind the point): %r" % (what, x))
        return Fraction(int(whole)) + (Fraction(int(frac), 10 ** len(frac)) if point else 0)
    return Fraction(x)


def ee_units(x):
    """Expected errors as the trim calls take them: floor(x * 2^32) of an int, a Fraction, or a decimal text of digits with at most one
    point that has 1 to 9 digits behind it ("2", "0.5", "1.999999999").  No floats: a float is not the number that was written."""
    v = int(_decimal(x, "a number of expected errors", "expected errors are") * 2 ** 32)
    if not 0 <= v < 2 ** 64 - 1:
        raise ValueError("expected errors out of range: %r" % (x,))
    return v


def trim_to_segments(rows):
    """The (record, begin, end) tuples unnaf_select_reads takes: the kept rows of the table unnaf_trim returns, in its order."""
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) == TRIM_KEPT]


def clip_budgets(rate, m):
    """Host-only: the 33 budgets of an adapter of m letters at an error rate (naf_gpu_clip_budgets): floor(L * rate) mismatches in an
    overlap of L <= m letters, at most L - 1, and 0 above m, as a list of ints.  rate: text ("0.1"), int or Fraction, never a float."""
    r = _decimal(rate, "an error rate", "an error rate is")
    if r < 0 or r.numerator >= 2 ** 64 or r.denominator >= 2 ** 64 or not 1 <= int(m) <= 32:
        raise ValueError("not an error rate and an adapter length of 1 to 32: %r, %r" % (rate, m))
    out = (C.c_uint8 * 33)()
    if load().naf_gpu_clip_budgets(r.numerator, r.denominator, int(m), out):
        raise ValueError("not an error rate and an adapter length of 1 to 32: %r, %r" % (rate, m))
    return [int(v) for v in out]


def clip_to_segments(rows):
    """The (record, begin, end) tuples unnaf_select_reads takes: the kept rows of the table unnaf_clip returns, in its order."""
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & TRIM_KEPT]


def dedup_level(copies):
    """Host-only: FastQC's duplication-level bin of a class of `copies` reads (naf_gpu_dedup_level): 0 to 8 for 1 to 9 copies, then 10-49,
    50-99, 100-499, 500-999, 1000-4999, 5000-9999 and 10000 or more as 9 to 15.  ValueError for 0."""
    v = C.c_uint()
    if not 0 < int(copies) < 2 ** 64 or load().naf_gpu_dedup_level(int(copies), C.byref(v)):
        raise ValueError("not a number of copies (1 or more): %r" % (copies,))
    return int(v.value)


def dedup_to_segments(rows):
    """The (record, begin, end) tuples unnaf_select_reads takes: the firsts of the table unnaf_dedup returns, in its order."""
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & TRIM_KEPT]


def screen_to_segments(rows):
    """The (record, begin, end) tuples unnaf_select_reads takes: the kept reads of the table unnaf_screen returns, in its order."""
    return [(int(x["record"]), int(x["begin"]), int(x["end"])) for x in rows if int(x["flags"]) & TRIM_KEPT]


def parse_base_class(text):
    """Host-only: the 16-bit set of a base class (naf_gpu_parse_base_class) -- bit c for 4-bit code c of "-TGKCYSBAWRDMHVN"; letters of
    ACGTU RYSWKM BDHV N and '-' in either case, a leading '^' complements.  ValueError for what is no class."""
    b = _text_arg(text, "a base class")
    s = C.c_uint16()
    if load().naf_gpu_parse_base_class(b, C.byref(s)):
        raise ValueError("not a base class: %r" % (text,))
    return s.value


def kmer_index(text, canonical=False):
    """Host-only: (k, index) of a k-mer of 1 to 12 letters of ACGTU in either case (naf_gpu_kmer_index): A = 0, C = 1, G = 2, T/U = 3,
    the first base the most significant; canonical: the smaller of the index and that of the reverse complement.  ValueError for
    anything else."""
    b = _text_arg(text, "a k-mer")
    k, idx = C.c_uint(), C.c_uint64()
    if load().naf_gpu_kmer_index(b, 1 if canonical else 0, C.byref(k), C.byref(idx)):
        raise ValueError("not a k-mer: %r" % (text,))
    return k.value, idx.value


def kmer_text(k, index):
    """Host-only: the k letters (ACGT) of index `index` among the 4**k k-mers (naf_gpu_kmer_text).  ValueError for k outside 1..12 or an
    index that is not below 4**k."""
    if not (isinstance(k, int) and isinstance(index, int) and 0 <= k < 2 ** 32 and 0 <= index < 2 ** 64):
        raise ValueError("not a k-mer: k %r index %r" % (k, index))
    out = C.create_string_buffer(13)
    if load().naf_gpu_kmer_text(k, index, out):
        raise ValueError("not a k-mer: k %r index %r" % (k, index))
    return out.value.decode()


def parse_codon_set(text):
    """Host-only: the 64-bit set of a comma-separated list of codons (naf_gpu_parse_codon_set) -- bit i for the codon of index i under
    kmer_index at K = 3 --; three letters each, either case, U = T, the IUPAC letters RYSWKM BDHV N expand.  ValueError for anything else."""
    b = _text_arg(text, "a list of codons")
    s = C.c_uint64()
    if load().naf_gpu_parse_codon_set(b, C.byref(s)):
        raise ValueError("not a list of codons: %r" % (text,))
    return s.value


def genetic_code(id_or_letters=1):
    """Host-only: a GeneticCode from an NCBI table number (naf_gpu_genetic_code_by_id: 1 .. 6, 9 .. 16, 21 .. 26) or from 64 letters A .. Z
    or '*' in the order AAA AAC AAG AAT ACA ... TTT (naf_gpu_genetic_code_parse); a GeneticCode is returned as it is.  ValueError for
    anything else."""
    if isinstance(id_or_letters, GeneticCode):
        return id_or_letters
    g = GeneticCode()
    if isinstance(id_or_letters, int) and not isinstance(id_or_letters, bool):
        if not -2 ** 31 <= id_or_letters < 2 ** 31 or load().naf_gpu_genetic_code_by_id(id_or_letters, C.byref(g)):
            raise ValueError("not a genetic code: %r" % (id_or_letters,))
        return g
    if not isinstance(id_or_letters, (str, bytes)):
        raise ValueError("not a genetic code: %r" % (id_or_letters,))
    if load().naf_gpu_genetic_code_parse(_text_arg(id_or_letters, "a genetic code"), C.byref(g)):
        raise ValueError("not a genetic code: %r" % (id_or_letters,))
    return g


def codon_lut(code=1):
    """Host-only: the 4096 letters of naf_gpu_codon_lut as bytes -- index (c0 << 8) | (c1 << 4) | c2 of the stored 4-bit codes of
    "-TGKCYSBAWRDMHVN" in reading order."""
    g = genetic_code(code)
    out = (C.c_uint8 * 4096)()
    if load().naf_gpu_codon_lut(C.byref(g), out):
        raise ValueError("not a genetic code: %r" % (code,))
    return bytes(out)


def genetic_code_stops(code=1):
    """Host-only: the codon set of a code's stops (naf_gpu_genetic_code_stops), as unnaf_orfs takes it."""
    g = genetic_code(code)
    s = C.c_uint64()
    if load().naf_gpu_genetic_code_stops(C.byref(g), C.byref(s)):
        raise ValueError("not a genetic code: %r" % (code,))
    return s.value


def frames_to_segments(lengths, frames, records=None):
    """The (record, begin, end, reverse) tuples unnaf_translate takes for the reading frames `frames` (out of 1, 2, 3, -1, -2, -3) of whole
    records: `lengths` are the records' lengths from record 0 on, `records` the record numbers to take (None: all), and the frames of one
    record stand side by side in the order listed.  Frame f > 0 is the record from base f - 1 on; frame -f its reverse complement from
    base f - 1 on, which is forward bases [0, length - (f - 1)) with reverse = 1 (ORFfinder's and seqkit's numbering, as in unnaf_orfs).
    Frames 1 and -1 are the whole record, (record, 0, WHOLE, reverse); a frame that has no base is left out."""
    out = []
    for r in (range(len(lengths)) if records is None else records):
        n = int(lengths[r])
        for f in frames:
            if f not in (1, 2, 3, -1, -2, -3):
                raise ValueError("not a reading frame: %r" % (f,))
            skip = abs(f) - 1
            if skip == 0:
                out.append((r, 0, WHOLE, 1 if f < 0 else 0))
            elif skip < n:
                out.append((r, skip, n, 0) if f > 0 else (r, 0, n - skip, 1))
    return out


def orfs_to_segments(rows, include_stop=False):
    """The (record, begin, end, reverse) tuples unnaf_select takes, one per open reading frame (rows of the table unnaf_orfs returns):
    selected, they are the coding texts in reading direction.  include_stop: the stop codon too, on the 3' side (behind `end` on strand
    0, in front of `begin` on strand 1), for the rows that have one (ORF_STOP3)."""
    out = []
    for x in rows:
        r, b, e, s = int(x["record"]), int(x["begin"]), int(x["end"]), int(x["strand"])
        if include_stop and int(x["flags"]) & ORF_STOP3:
            if s:
                b -= 3
            else:
                e += 3
        out.append((r, b, e, s))
    return out


def runs_to_segments(runs, flank=0, lengths=None):
    """The (record, begin, end) tuples unnaf_select takes, one per run (rows of the table unnaf_runs returns).  flank: that many bases
    more on either side, clamped to the record -- to its start always, to its end when `lengths` (the n_bases of unnaf_record_table,
    indexed by record number) is given; unnaf_select clamps an end beyond the record itself."""
    out = []
    for x in runs:
        r, b, e = int(x["record"]), max(0, int(x["begin"]) - flank), int(x["end"]) + flank
        if lengths is not None:
            e = min(e, int(lengths[r]))
        out.append((r, b, e))
    return out


def parse_repeat_spec(text):
    """Host-only: the sixteen min_copies of a repeat spec in MISA's definition syntax -- "1-10,2-6,3-5", or the word "misa"
    (naf_gpu_parse_repeat_spec) -- as a list, [p - 1] for period p, 0 where the period is not searched.  ValueError for what is no spec."""
    sp = RepeatSpec()
    if load().naf_gpu_parse_repeat_spec(_text_arg(text, "a repeat spec"), C.byref(sp)):
        raise ValueError("not a repeat spec: %r" % (text,))
    return [int(v) for v in sp.min_copies]


def repeat_class(motif, period):
    """Host-only: the motif class (naf_gpu_repeat_class) -- the smallest, in A < C < G < T order, of the rotations of the motif and of its
    reverse complement, in the row's encoding.  ValueError for a period outside 1 .. 16 or motif bits above 2 * period."""
    out = C.c_uint32()
    if not (0 <= int(motif) < 2 ** 32 and 0 <= int(period) < 2 ** 32) or load().naf_gpu_repeat_class(int(motif), int(period), C.byref(out)):
        raise ValueError("not a motif: %r of period %r" % (motif, period))
    return out.value


def repeat_motif_text(motif, period, rna=False):
    """The `period` letters of a row's motif, upper case; rna: U for T."""
    if not 1 <= int(period) <= 16 or int(motif) >> (2 * int(period)):
        raise ValueError("not a motif: %r of period %r" % (motif, period))
    return "".join(("ACGU" if rna else "ACGT")[(int(motif) >> (2 * k)) & 3] for k in range(int(period)))


def repeats_to_segments(rows, flank=0, lengths=None):
    """The (record, begin, end) tuples unnaf_select takes, one per tandem repeat (rows of the table unnaf_repeats returns).  flank: that
    many bases more on either side, clamped to the record -- to its start always, to its end when `lengths` (the n_bases of
    unnaf_record_table, indexed by record number) is given; unnaf_select clamps an end beyond the record itself."""
    return runs_to_segments(rows, flank, lengths)


def hits_to_segments(hits, patterns, flank=0, lengths=None):
    """The (record, begin, end, reverse) tuples unnaf_select takes, one per hit (rows of the table unnaf_locate or unnaf_locate_near
    returns), for the patterns the search was made with; brackets do not count for a pattern's length.  flank: that many bases more on either side, clamped to the record -- to its start always, to its end when
    `lengths` (the n_bases of unnaf_record_table, indexed by record number) is given; unnaf_select clamps an end beyond the record itself."""
    out = []
    for h in hits:
        r, b, e = int(h["record"]), int(h["begin"]), int(h["begin"]) + len(motif_letters(patterns[int(h["pattern"])]))
        b, e = max(0, b - flank), e + flank
        if lengths is not None:
            e = min(e, int(lengths[r]))
        out.append((r, b, e, int(h["strand"])))
    return out


def shard_carry(infos, k):
    """Host-only: what shard k's finish applies on behalf of its neighbours (naf_gpu_ennaf_shard_carry)."""
    L = load()
    arr = (ShardInfo * len(infos))(*infos)
    out = ShardCarry()
    rc = L.naf_gpu_ennaf_shard_carry(arr, len(infos), k, C.byref(out))
    if rc:
        raise NafGpuError(rc, L.naf_gpu_strerror(rc).decode())
    return out


def stitch_plan(opts, infos, pieces):
    """Host-only: (segments, literal bytes, archive length, report) of the joined archive (naf_gpu_ennaf_stitch_plan)."""
    L = load()
    n = len(infos)
    ia = (ShardInfo * n)(*infos)
    pa = (ShardPieces * n)(*pieces)
    segs = (StitchSeg * (7 + 6 * n))()
    title = opts.title or b""
    lit = C.create_string_buffer(256 + len(title))
    ns, ll, nl = C.c_size_t(), C.c_size_t(), C.c_uint64()
    rep = EnnafReport()
    rc = L.naf_gpu_ennaf_stitch_plan(C.byref(opts), ia, pa, n, segs, len(segs), C.byref(ns), lit, len(lit), C.byref(ll), C.byref(nl), C.byref(rep))
    if rc:
        raise NafGpuError(rc, L.naf_gpu_strerror(rc).decode())
    return [segs[k] for k in range(ns.value)], lit.raw[:ll.value], nl.value, rep


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _SyncedLib:
    """The library as a Context sees it.  The library reads its NAF_GPU_* switches from the environment once, in naf_gpu_init, and
    afterwards only through naf_gpu_set_option; tests and tools flip switches between calls by changing os.environ, so every entry point
    taken through this proxy first hands the library what changed since the last one (a NAF_GPU_DEBUG_* variable turns TRACE on), and a
    trace a call left is written to stderr when the call returns -- where the tests read which path ran."""

    def __init__(self, lib, ctx):
        object.__setattr__(self, "_lib", lib)
        object.__setattr__(self, "_ctx", ctx)

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        ctx = self._ctx
        if not ctx.h or name in ("naf_gpu_set_option", "naf_gpu_get_trace", "naf_gpu_clear_trace", "naf_gpu_last_error", "naf_gpu_strerror", "naf_gpu_shutdown"):
            return f
        ctx._sync_options()
        if not ctx._tracing:
            return f

        def traced(*a):
            try:
                return f(*a)
            finally:
                t = self._lib.naf_gpu_get_trace(ctx.h)
                if t:
                    os.write(2, t)
                    self._lib.naf_gpu_clear_trace(ctx.h)
        return traced


def _env_options():
    o = {k[8:]: v for k, v in os.environ.items() if k.startswith("NAF_GPU_")}
    if any(k.startswith("DEBUG_") for k in o) and "TRACE" not in o:
        o["TRACE"] = "1"
    return o


class Context:
    """One per device / per process rank.  Work is enqueued on torch's current stream for the device."""

    def __init__(self, device=0, use_torch_stream=True):
        import torch
        self.h = C.c_void_p()
        self._opts = {}
        self._tracing = False
        self.L = _SyncedLib(load(), self)
        rc = load().naf_gpu_init(device, C.byref(self.h))
        if rc:
            raise NafGpuError(rc, load().naf_gpu_strerror(rc).decode())
        self._opts = {k[8:]: v for k, v in os.environ.items() if k.startswith("NAF_GPU_")}      # what naf_gpu_init has read
        self.device = torch.device("cuda", device)
        if use_torch_stream:
            s = torch.cuda.current_stream(self.device)
            self._check(self.L.naf_gpu_set_stream(self.h, C.c_void_p(s.cuda_stream)))

    def close(self):
        if self.h:
            self.L.naf_gpu_shutdown(self.h)
            self.h = C.c_void_p()

    def set_option(self, name, value):
        """naf_gpu_set_option: one switch of this context (value None: not set)."""
        self._check(load().naf_gpu_set_option(self.h, name.encode(), None if value is None else str(value).encode()))

    def _sync_options(self):
        # (os.environ is looked through per call: cheap beside a call, but not inside a timed loop of short ones -- the raw items are
        # compared first, the dictionary work only when one of them changed)
        key = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("NAF_GPU_")))
        if key == getattr(self, "_opts_key", None):
            return
        self._opts_key = key
        want = _env_options()
        if want != self._opts:
            for k in set(self._opts) - set(want):
                self.set_option(k, None)
            for k, v in want.items():
                if self._opts.get(k) != v:
                    self.set_option(k, v)
            self._opts = want
        self._tracing = want.get("TRACE", "")[:1] == "1"

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise NafGpuError(rc, self.L.naf_gpu_last_error(self.h).decode("latin1"))

    def to_device(self, data: bytes):
        import torch
        import numpy as np
        if len(data) == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device)
        return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.device)

    def reserve(self, nbytes):
        self._check(self.L.naf_gpu_reserve(self.h, nbytes))

    def write_file(self, fd, file_off, t):
        """naf_gpu_write_file: the bytes of device tensor t at file_off of descriptor fd (a regular file)."""
        self._check(self.L.naf_gpu_write_file(self.h, int(fd), C.c_uint64(int(file_off)), _ptr(t), int(t.numel())))

    def release_scratch(self):
        """Give the context's scratch arenas back to the device (the next call grows them again)."""
        self._check(self.L.naf_gpu_release_scratch(self.h))

    def set_stream(self, stream):
        """naf_gpu_set_stream: a torch.cuda.Stream, a raw hipStream_t as an int, or None for HIP's null stream."""
        s = getattr(stream, "cuda_stream", stream)
        self._check(self.L.naf_gpu_set_stream(self.h, C.c_void_p(s or None)))

    def mem_info(self):
        """(free, total) bytes of the device as the runtime sees them now (naf_gpu_mem_info)."""
        fr, tot = C.c_size_t(), C.c_size_t()
        self._check(self.L.naf_gpu_mem_info(self.h, C.byref(fr), C.byref(tot)))
        return fr.value, tot.value

    def host_alloc(self, nbytes):
        """naf_gpu_host_alloc: the address of nbytes of pinned host memory (host_free gives it back)."""
        p = C.c_void_p()
        self._check(self.L.naf_gpu_host_alloc(self.h, int(nbytes), C.byref(p)))
        return p.value

    def host_free(self, addr):
        self._check(self.L.naf_gpu_host_free(self.h, C.c_void_p(addr)))

    def upload(self, t, h_src, nbytes):
        """naf_gpu_upload: nbytes from host address h_src into device tensor t, asynchronous on the stream."""
        self._check(self.L.naf_gpu_upload(self.h, _ptr(t), C.c_void_p(h_src), int(nbytes)))

    def download(self, h_dst, t, nbytes):
        """naf_gpu_download: nbytes of device tensor t to host address h_dst; returns after completion."""
        self._check(self.L.naf_gpu_download(self.h, C.c_void_p(h_dst), _ptr(t), int(nbytes)))

    def download_async(self, h_pinned, t, nbytes):
        """naf_gpu_download_async: the same into pinned memory without waiting; pair with synchronize()."""
        self._check(self.L.naf_gpu_download_async(self.h, C.c_void_p(h_pinned), _ptr(t), int(nbytes)))

    def copy(self, dst, src, nbytes):
        """naf_gpu_copy: device to device, asynchronous on the stream."""
        self._check(self.L.naf_gpu_copy(self.h, _ptr(dst), _ptr(src), int(nbytes)))

    def read_file(self, fd, file_off, t, nbytes=None):
        """naf_gpu_read_file: bytes [file_off, file_off + nbytes) of descriptor fd (a regular file) into device tensor t."""
        self._check(self.L.naf_gpu_read_file(self.h, int(fd), C.c_uint64(int(file_off)), int(t.numel() if nbytes is None else nbytes), _ptr(t)))

    def write_fd(self, fd, t):
        """naf_gpu_write_fd: the bytes of device tensor t to a descriptor that is written in order (a pipe, an O_APPEND file)."""
        self._check(self.L.naf_gpu_write_fd(self.h, int(fd), _ptr(t), int(t.numel())))

    def gather_ranges(self, out, parts):
        """naf_gpu_gather_ranges: parts = [(ctx, tensor, dst_offset)] -- every part is pushed into `out` (a tensor on this context's
        device) by its own context's stream; this context's stream waits for all of them."""
        n = len(parts)
        srcs = (C.c_void_p * n)(*[p[0].h.value for p in parts])
        ptrs = (C.c_void_p * n)(*[p[1].data_ptr() for p in parts])
        offs = (C.c_uint64 * n)(*[int(p[2]) for p in parts])
        lens = (C.c_size_t * n)(*[int(p[1].numel()) for p in parts])
        self._check(self.L.naf_gpu_gather_ranges(self.h, _ptr(out), srcs, ptrs, offs, lens, n))

    # ---- zstd ----
    def zstd_decompress(self, d_frame, out_cap, has_magic=True):
        import torch
        out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_zstd_decompress(self.h, _ptr(d_frame), d_frame.numel(), int(has_magic), _ptr(out), out_cap, C.byref(n)))
        return out[:n.value]

    def zstd_compress(self, d_src, level=1):
        import torch
        cap = self.L.naf_gpu_zstd_compress_bound(d_src.numel())
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_zstd_compress(self.h, _ptr(d_src), d_src.numel(), level, _ptr(out), cap, C.byref(n)))
        return out[:n.value]

    # ---- unnaf ----
    def parse_header(self, d_naf):
        h = Header()
        self._check(self.L.naf_gpu_parse_header(self.h, _ptr(d_naf), d_naf.numel(), C.byref(h)))
        return h

    def unnaf_size(self, d_naf, out_type=OUT_DEFAULT, use_mask=True, line_length=-1):
        o = UnnafOpts(out_type, int(use_mask), line_length)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_unnaf_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(n)))
        return n.value

    def unnaf(self, d_naf, out_type=OUT_DEFAULT, use_mask=True, line_length=-1, out=None):
        import torch
        o = UnnafOpts(out_type, int(use_mask), line_length)
        if out is None:
            size = self.unnaf_size(d_naf, out_type, use_mask, line_length)
            out = torch.empty(max(size, 1), dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_unnaf(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), _ptr(out), out.numel(), C.byref(n)))
        return out[:n.value]

    def unnaf_range(self, d_naf, begin, end, out_type=OUT_DEFAULT, use_mask=True, line_length=-1, out=None):
        import torch
        o = UnnafOpts(out_type, int(use_mask), line_length)
        if out is None:
            out = torch.empty(max(end - begin, 1), dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_unnaf_range(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), begin, end, _ptr(out), out.numel(), C.byref(n)))
        return out[:n.value]

    def unnaf_find(self, d_naf, ids):
        """Record numbers of the given ids (str or bytes): the first record whose id equals each one, None where there is none."""
        raw = [i.encode("latin1") if isinstance(i, str) else bytes(i) for i in ids]
        if any(b"\0" in i for i in raw):
            raise ValueError("an id cannot hold a zero byte")
        blob = b"".join(i + b"\0" for i in raw)
        rec = (C.c_uint64 * max(len(raw), 1))()
        self._check(self.L.naf_gpu_unnaf_find(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), len(raw), rec))
        return [None if rec[k] == WHOLE else int(rec[k]) for k in range(len(raw))]

    def unnaf_record_table(self, d_naf, first=0, count=None, out_type=OUT_DEFAULT, use_mask=True, line_length=-1):
        """(n_bases, text_off) of records [first, first + count): text_off has count + 1 entries, consecutive pairs are what
        unnaf_range takes for a record.  count=None: up to the last record."""
        o = UnnafOpts(out_type, int(use_mask), line_length)
        if count is None:
            count = int(self.parse_header(d_naf).n_sequences) - first
        nb, off = (C.c_uint64 * max(count, 1))(), (C.c_uint64 * (count + 1))()
        self._check(self.L.naf_gpu_unnaf_record_table(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), first, count, nb, off))
        return [int(nb[k]) for k in range(count)], [int(off[k]) for k in range(count + 1)]

    @staticmethod
    def _segments(segments):
        segs = (Segment * max(len(segments), 1))()
        for k, s in enumerate(segments):
            segs[k] = Segment(int(s), 0, WHOLE) if isinstance(s, int) else Segment(int(s[0]), int(s[1]), int(s[2]))
        return segs

    @staticmethod
    def _strands(segments):
        """The strand bytes of a list that holds 4-tuples (record, begin, end, reverse); None when it holds none."""
        if not any(not isinstance(s, int) and len(s) == 4 for s in segments):
            return None
        st = (C.c_uint8 * len(segments))()
        for k, s in enumerate(segments):
            if not isinstance(s, int) and len(s) == 4:
                st[k] = int(s[3])
        return st

    def _select_size(self, d_naf, o, segs, strands, n_segs, n):
        if strands is None:
            self._check(self.L.naf_gpu_unnaf_select_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, n_segs, C.byref(n)))
        else:
            self._check(self.L.naf_gpu_unnaf_select_stranded_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, strands, n_segs, C.byref(n)))

    def unnaf_select_size(self, d_naf, segments, out_type=OUT_DEFAULT, use_mask=True, line_length=-1):
        o = UnnafOpts(out_type, int(use_mask), line_length)
        n = C.c_size_t()
        self._select_size(d_naf, o, self._segments(segments), self._strands(segments), len(segments), n)
        return n.value

    def unnaf_select(self, d_naf, segments, out_type=OUT_DEFAULT, use_mask=True, line_length=-1, out=None):
        """The texts of the segments -- (record, begin, end) tuples, 0-based half-open, or record numbers for whole records -- laid
        end to end in the order given (naf_gpu_unnaf_select).  A 4-tuple (record, begin, end, reverse) gives a strand: reverse = 1 is
        the segment's reverse complement; a list that holds one goes through naf_gpu_unnaf_select_stranded."""
        import torch
        o = UnnafOpts(out_type, int(use_mask), line_length)
        segs, strands = self._segments(segments), self._strands(segments)
        n = C.c_size_t()
        if out is None:
            self._select_size(d_naf, o, segs, strands, len(segments), n)
            out = torch.empty(max(n.value, 1), dtype=torch.uint8, device=self.device)
        if strands is None:
            self._check(self.L.naf_gpu_unnaf_select(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, len(segments), _ptr(out), out.numel(), C.byref(n)))
        else:
            self._check(self.L.naf_gpu_unnaf_select_stranded(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, strands, len(segments), _ptr(out), out.numel(), C.byref(n)))
        return out[:n.value]

    def unnaf_select_reads_size(self, d_naf, segments, out_type=OUT_DEFAULT, use_mask=True, line_length=-1):
        o = UnnafOpts(out_type, int(use_mask), line_length)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_unnaf_select_reads_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), self._segments(segments), self._strands(segments), len(segments), C.byref(n)))
        return n.value

    def unnaf_select_reads(self, d_naf, segments, out_type=OUT_DEFAULT, use_mask=True, line_length=-1, out=None):
        """The texts of the segments as READS (naf_gpu_unnaf_select_reads): what unnaf_select gives, 3- and 4-tuples alike, except that a
        sub-range keeps the header line of its whole record ("/rc" behind the id for a reverse one) and so can be written as FASTQ: bases
        and quality codes [begin, end).  trim_to_segments gives the segments of a trim table's kept rows."""
        import torch
        o = UnnafOpts(out_type, int(use_mask), line_length)
        segs, strands = self._segments(segments), self._strands(segments)
        n = C.c_size_t()
        if out is None:
            self._check(self.L.naf_gpu_unnaf_select_reads_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, strands, len(segments), C.byref(n)))
            out = torch.empty(max(n.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.L.naf_gpu_unnaf_select_reads(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), segs, strands, len(segments), _ptr(out), out.numel(), C.byref(n)))
        return out[:n.value]

    def unnaf_translate_size(self, d_naf, segments, code=1, line_length=-1):
        o = UnnafOpts(OUT_FASTA, 0, line_length)
        g = genetic_code(code)
        n = C.c_size_t()
        self._check(self.L.naf_gpu_unnaf_translate_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(g), self._segments(segments), self._strands(segments), len(segments), C.byref(n)))
        return n.value

    def unnaf_translate(self, d_naf, segments, code=1, line_length=-1, out=None):
        """The segments as protein FASTA (naf_gpu_unnaf_translate): per segment -- as unnaf_select takes them, 4-tuples for strands -- the
        header line unnaf_select writes in FASTA mode, then floor(bases / 3) letters read from the segment's first base in reading
        direction, wrapped at line_length letters (-1: the archive's line length, 0: one line).  code: an NCBI table number, 64 letters or
        a GeneticCode."""
        import torch
        o = UnnafOpts(OUT_FASTA, 0, line_length)
        g = genetic_code(code)
        segs, strands = self._segments(segments), self._strands(segments)
        n = C.c_size_t()
        if out is None:
            self._check(self.L.naf_gpu_unnaf_translate_size(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(g), segs, strands, len(segments), C.byref(n)))
            out = torch.empty(max(n.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.L.naf_gpu_unnaf_translate(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), C.byref(g), segs, strands, len(segments), _ptr(out), out.numel(), C.byref(n)))
        return out[:n.value]

    def _guessed_table(self, call, n, row_bytes, dtype, out):
        """The table of rows that `call(tensor, capacity in rows)` writes, leaving the number of rows in `n` and returning the library's
        code.  out: the caller's uint8 device tensor takes it, and the torch view of the bytes written is returned.  Without it the rows
        come back as a structured numpy array, from a table sized by a guess of 4096 rows first and by the whole number when that was
        too small (the call reports it with E_CAP)."""
        import numpy as np
        import torch
        if out is not None:
            self._check(call(out, out.numel() // row_bytes))
            return out[:row_bytes * n.value]
        cap = 4096
        buf = torch.empty(row_bytes * cap, dtype=torch.uint8, device=self.device)
        rc = call(buf, cap)
        if rc == E_CAP:
            cap = n.value
            buf = torch.empty(row_bytes * cap, dtype=torch.uint8, device=self.device)
            rc = call(buf, cap)
        self._check(rc)
        return np.frombuffer(buf[:row_bytes * n.value].cpu().numpy().tobytes(), dtype=dtype)

    def _counted_table(self, count, call, n, row_bytes, dtype, out):
        """As _guessed_table, for a table that is counted first: without `out`, `count()` leaves the number of rows in `n` and the
        table is made that large."""
        import numpy as np
        import torch
        if out is not None:
            self._check(call(out, out.numel() // row_bytes))
            return out[:row_bytes * n.value]
        self._check(count())
        buf = torch.empty(max(row_bytes * n.value, 1), dtype=torch.uint8, device=self.device)
        self._check(call(buf, n.value))
        return np.frombuffer(buf[:row_bytes * n.value].cpu().numpy().tobytes(), dtype=dtype)

    @staticmethod
    def _patterns(patterns):
        raw = [p.encode("latin1") if isinstance(p, str) else bytes(p) for p in patterns]
        if any(b"\0" in p for p in raw):
            raise ValueError("a pattern cannot hold a zero byte")
        return b"".join(p + b"\0" for p in raw), len(raw)

    def unnaf_locate_count(self, d_naf, patterns, strands=3, first=0, count=None):
        """(hits in all, [[forward, reverse] per pattern]) of IUPAC patterns in records [first, first + count) -- count=None: to the last
        record; strands: 1 as stored, 2 reverse, 3 both (naf_gpu_unnaf_locate_count)."""
        blob, n = self._patterns(patterns)
        total, per = C.c_uint64(), (C.c_uint64 * max(2 * n, 1))()
        self._check(self.L.naf_gpu_unnaf_locate_count(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, int(strands), int(first),
                                                      WHOLE if count is None else int(count), C.byref(total), per))
        return total.value, [[int(per[2 * k]), int(per[2 * k + 1])] for k in range(n)]

    def unnaf_locate(self, d_naf, patterns, strands=3, first=0, count=None, out=None):
        """(hits, total): the hits as a structured numpy array (HIT_DTYPE: record, begin, pattern, strand) in the order of the contract --
        (record, begin), pattern number, strand.  out: a uint8 device tensor to take the table (24 bytes a hit); then `hits` is the torch
        view of its first 24 * total bytes and too small a tensor raises NafGpuError(E_CAP).  Without it the table is counted first."""
        blob, n = self._patterns(patterns)
        total = C.c_uint64()
        cnt = WHOLE if count is None else int(count)

        def counted():
            return self.L.naf_gpu_unnaf_locate_count(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, int(strands), int(first), cnt, C.byref(total), None)

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_locate(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, int(strands), int(first), cnt, _ptr(buf), cap, C.byref(total))
        hits = self._counted_table(counted, call, total, 24, HIT_DTYPE, out)
        return hits, total.value

    @staticmethod
    def _budgets(mismatches, n):
        try:
            vals = [mismatches.__index__()] * n                                   # one for all patterns (any integer type)
        except (AttributeError, TypeError):
            vals = list(mismatches)                                               # or one each
        if len(vals) != n:
            raise ValueError("%d budgets of mismatches for %d patterns" % (len(vals), n))
        if any(not 0 <= int(v) < 2 ** 32 for v in vals):
            raise ValueError("a budget of mismatches is a uint32_t (the library accepts 0 to %d and names the pattern of any other)" % LOCATE_MAX_MISMATCHES)
        return (C.c_uint32 * max(n, 1))(*[int(v) for v in vals])

    def unnaf_locate_near_count(self, d_naf, patterns, mismatches, strands=3, first=0, count=None):
        """(hits in all, [[forward, reverse] per pattern], each a list of 9 counts by number of mismatches) of IUPAC patterns within
        their budget of mismatches -- one int for all patterns or one per pattern; letters in square brackets must match
        (naf_gpu_unnaf_locate_near_count).  The rest as unnaf_locate_count."""
        blob, n = self._patterns(patterns)
        total, per = C.c_uint64(), (C.c_uint64 * max(18 * n, 1))()
        self._check(self.L.naf_gpu_unnaf_locate_near_count(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, self._budgets(mismatches, n), int(strands), int(first),
                                                           WHOLE if count is None else int(count), C.byref(total), per))
        return total.value, [[[int(per[(2 * k + s) * 9 + d]) for d in range(9)] for s in (0, 1)] for k in range(n)]

    def unnaf_locate_near(self, d_naf, patterns, mismatches, strands=3, first=0, count=None, out=None):
        """(hits, total): the near hits as a structured numpy array (NEAR_HIT_DTYPE: record, begin, pattern, strand, mismatches, where) in
        the order of the contract.  out: a uint8 device tensor to take the table (32 bytes a hit); then `hits` is the torch view of its
        first 32 * total bytes and too small a tensor raises NafGpuError(E_CAP).  Without it the table is counted first."""
        blob, n = self._patterns(patterns)
        budgets = self._budgets(mismatches, n)
        total = C.c_uint64()
        cnt = WHOLE if count is None else int(count)

        def counted():
            return self.L.naf_gpu_unnaf_locate_near_count(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, budgets, int(strands), int(first), cnt, C.byref(total), None)

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_locate_near(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), n, budgets, int(strands), int(first), cnt, _ptr(buf), cap, C.byref(total))
        hits = self._counted_table(counted, call, total, 32, NEAR_HIT_DTYPE, out)
        return hits, total.value

    def unnaf_composition_rows(self, d_naf, window=0, first=0, count=None):
        """The rows unnaf_composition gives for records [first, first + count) under `window` (naf_gpu_unnaf_composition_rows: the lengths
        only, no sequence is decoded)."""
        n = C.c_uint64()
        self._check(self.L.naf_gpu_unnaf_composition_rows(self.h, _ptr(d_naf), d_naf.numel(), int(window), int(first), WHOLE if count is None else int(count), C.byref(n)))
        return n.value

    def unnaf_composition(self, d_naf, window=0, mask=True, first=0, count=None, out=None):
        """(rows, total): the base composition of records [first, first + count) -- one row per record (window 0) or per window of
        `window` bases -- as a structured numpy array (COMP_DTYPE: record, begin, end, n[16], masked, cpg), and their sum as a CompRow
        (its record: the records covered, its end: their bases).  mask: count the soft-masked bases (NAF_GPU_COMP_MASK).  out: a uint8
        device tensor to take the table (168 bytes a row); then `rows` is the torch view of its first 168 * n bytes and too small a
        tensor raises NafGpuError(E_CAP).  Without it the rows are counted first (naf_gpu_unnaf_composition_rows)."""
        n, tot = C.c_uint64(), CompRow()
        cnt = WHOLE if count is None else int(count)
        flags = COMP_MASK if mask else 0

        def counted():
            return self.L.naf_gpu_unnaf_composition_rows(self.h, _ptr(d_naf), d_naf.numel(), int(window), int(first), cnt, C.byref(n))

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_composition(self.h, _ptr(d_naf), d_naf.numel(), int(window), flags, int(first), cnt, _ptr(buf), cap, C.byref(n), C.byref(tot))
        rows = self._counted_table(counted, call, n, COMP_ROW_BYTES, COMP_DTYPE, out)
        return rows, tot

    def unnaf_quality_rows(self, d_naf, cycle_bin=0, first=0, count=None):
        """(record rows, cycle rows) that unnaf_quality gives for records [first, first + count) under `cycle_bin`
        (naf_gpu_unnaf_quality_rows: the lengths only, no quality byte is decoded)."""
        nr, nc = C.c_uint64(), C.c_uint64()
        self._check(self.L.naf_gpu_unnaf_quality_rows(self.h, _ptr(d_naf), d_naf.numel(), int(cycle_bin), int(first), WHOLE if count is None else int(count),
                                                      C.byref(nr), C.byref(nc)))
        return nr.value, nc.value

    def unnaf_quality(self, d_naf, cycle_bin=0, first=0, count=None, records=True, cycles=None, out_records=None, out_cycles=None):
        """(rec_rows, cycle_rows, hist, total): the quality statistics of records [first, first + count) -- one row per read, and one per
        bin of `cycle_bin` read positions -- as structured numpy arrays (QUAL_DTYPE: key, n, sum, ee, n_q20, n_q30, min, max), the count
        per byte value as a list of 256 ints and the sum over all as a QualRow (its key: the records covered).  records / cycles: whether
        the table is wanted (cycles=None: when cycle_bin > 0); a table that is not wanted comes back as None.  out_records / out_cycles:
        uint8 device tensors to take the tables (56 bytes a row); that table is then the torch view of the bytes written, and too small
        a tensor raises NafGpuError(E_CAP).  Without them the rows are counted first (naf_gpu_unnaf_quality_rows)."""
        import numpy as np
        import torch
        cnt = WHOLE if count is None else int(count)
        W = int(cycle_bin)
        cycles = (W > 0) if cycles is None else (bool(cycles) and W > 0)
        nr, nc, tot, hist = C.c_uint64(), C.c_uint64(), QualRow(), (C.c_uint64 * 256)()
        if (records and out_records is None) or (cycles and out_cycles is None):
            self._check(self.L.naf_gpu_unnaf_quality_rows(self.h, _ptr(d_naf), d_naf.numel(), W, int(first), cnt, C.byref(nr), C.byref(nc)))
        bufs = []
        for want, out, n in ((records, out_records, nr.value), (cycles, out_cycles, nc.value)):
            if want and out is None:
                bufs.append((torch.empty(max(QUAL_ROW_BYTES * n, 1), dtype=torch.uint8, device=self.device), n, True))
            elif want:
                bufs.append((out, out.numel() // QUAL_ROW_BYTES, False))
            else:
                bufs.append((None, 0, False))
        (rb, rcap, rown), (cb, ccap, cown) = bufs
        self._check(self.L.naf_gpu_unnaf_quality(self.h, _ptr(d_naf), d_naf.numel(), W, int(first), cnt, _ptr(rb) if rb is not None else None, rcap,
                                                 _ptr(cb) if cb is not None else None, ccap, C.byref(nr), C.byref(nc), hist, C.byref(tot)))

        def table(buf, own, n):
            if buf is None:
                return None
            view = buf[:QUAL_ROW_BYTES * n]
            return np.frombuffer(view.cpu().numpy().tobytes(), dtype=QUAL_DTYPE) if own else view
        return table(rb, rown, nr.value), table(cb, cown, nc.value), [int(v) for v in hist], tot

    def unnaf_trim(self, d_naf, limit, min_len=1, max_ee=None, first=0, count=None, out=None):
        """(rows, total): the stretch to keep of every read of records [first, first + count) and what the filters say of it
        (naf_gpu_unnaf_trim) -- limit: the cutoff error rate times 2^32 (trim_limit(q) for Phred q; TRIM_NONE: no trimming); min_len: the
        bases a kept read needs; max_ee: the expected errors times 2^32 it may have (ee_units; None: any) -- as a structured numpy array
        (TRIM_DTYPE: record, begin, end, ee, flags, reserved), one row per read, and a TrimTotal.  out: a uint8 device tensor to take the
        table (40 bytes a row); then `rows` is the torch view of its first 40 * n bytes and too small a tensor raises NafGpuError(E_CAP).
        out=False: the totals only, rows is None."""
        import numpy as np
        import torch
        o = TrimOpts(int(limit), int(min_len), 2 ** 64 - 1 if max_ee is None else int(max_ee))
        n, tot = C.c_uint64(), TrimTotal()
        cnt = WHOLE if count is None else int(count)
        own = out is None
        if own:
            have = int(self.parse_header(d_naf).n_sequences)
            rows = max(0, min(have - int(first), cnt)) if cnt != WHOLE else max(0, have - int(first))
            out = torch.empty(max(TRIM_BYTES * rows, 1), dtype=torch.uint8, device=self.device)
        buf = None if out is False else out
        self._check(self.L.naf_gpu_unnaf_trim(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), int(first), cnt, _ptr(buf) if buf is not None else None,
                                              buf.numel() // TRIM_BYTES if buf is not None else 0, C.byref(n), C.byref(tot)))
        if buf is None:
            return None, tot
        view = buf[:TRIM_BYTES * n.value]
        return (np.frombuffer(view.cpu().numpy().tobytes(), dtype=TRIM_DTYPE) if own else view), tot

    def unnaf_clip(self, d_naf, adapters, rate="0.1", budgets=None, min_overlap=3, min_len=1, bounds=None, first=0, count=None, out=None):
        """(rows, total, per_adapter): where a 3' adapter begins in every read of records [first, first + count) (naf_gpu_unnaf_clip) --
        adapters: 1 to 16 IUPAC texts of 1 to 32 letters; rate: the mismatches allowed per overlapped letter (clip_budgets), or budgets:
        one table of 33 ints per adapter; min_overlap: the letters of an adapter that must lie in the read; min_len: the bases a kept
        read needs; bounds: a uint8 device tensor of trim rows for the same records (the view unnaf_trim(out=...) returned), whose
        (begin, end) are searched instead of the whole reads -- as a structured numpy array (CLIP_DTYPE), one row per read, a ClipTotal
        and the clips by [adapter][overlap] as lists of 33 ints.  out: a uint8 device tensor to take the table (40 bytes a row); then
        `rows` is the torch view of its first 40 * n bytes and too small a tensor raises NafGpuError(E_CAP).  out=False: the totals only."""
        import numpy as np
        import torch
        blob, na = self._patterns(adapters)
        if budgets is None:
            budgets = [clip_budgets(rate, min(max(len(a), 1), 32)) for a in adapters]
        flat = [int(v) for b in budgets for v in b]
        if len(flat) != 33 * na or any(not 0 <= v < 256 for v in flat):
            raise ValueError("budgets: 33 values of 0 to 255 per adapter")
        tab = (C.c_uint8 * max(len(flat), 1))(*flat)
        o = ClipOpts(int(min_overlap), int(min_len))
        n, tot, per = C.c_uint64(), ClipTotal(), (C.c_uint64 * max(33 * na, 1))()
        cnt = WHOLE if count is None else int(count)
        own = out is None
        if own:
            have = int(self.parse_header(d_naf).n_sequences)
            rows = max(0, min(have - int(first), cnt)) if cnt != WHOLE else max(0, have - int(first))
            out = torch.empty(max(CLIP_BYTES * rows, 1), dtype=torch.uint8, device=self.device)
        buf = None if out is False else out
        self._check(self.L.naf_gpu_unnaf_clip(self.h, _ptr(d_naf), d_naf.numel(), blob, len(blob), na, tab, C.byref(o), int(first), cnt,
                                              _ptr(bounds) if bounds is not None else None, _ptr(buf) if buf is not None else None,
                                              buf.numel() // CLIP_BYTES if buf is not None else 0, C.byref(n), C.byref(tot), per))
        per_adapter = [[int(per[33 * k + L]) for L in range(33)] for k in range(na)]
        if buf is None:
            return None, tot, per_adapter
        view = buf[:CLIP_BYTES * n.value]
        return (np.frombuffer(view.cpu().numpy().tobytes(), dtype=CLIP_DTYPE) if own else view), tot, per_adapter

    def unnaf_dedup(self, d_naf, both_strands=False, bounds=None, bounds_kind="trim", first=0, count=None, out=None):
        """(rows, total, levels): the classes of equal reads among records [first, first + count) (naf_gpu_unnaf_dedup) -- both_strands: a
        read and its reverse complement are one class; bounds: a uint8 device tensor of the rows unnaf_trim (bounds_kind "trim") or
        unnaf_clip ("clip") wrote for the same records, whose (begin, end) are compared instead of the whole reads and whose rows
        without TRIM_KEPT take no part -- as a structured numpy array (DEDUP_DTYPE), one row per read, a DedupTotal and the classes by
        FastQC's duplication level as a list of DEDUP_LEVELS ints.  out: a uint8 device tensor to take the table (48 bytes a row); then
        `rows` is the torch view of its first 48 * n bytes and too small a tensor raises NafGpuError(E_CAP).  out=False: the totals only."""
        import numpy as np
        import torch
        kinds = {"trim": DEDUP_BOUNDS_TRIM, "clip": DEDUP_BOUNDS_CLIP}
        if bounds_kind not in kinds and not isinstance(bounds_kind, int):
            raise ValueError("bounds_kind: 'trim' or 'clip', not %r" % (bounds_kind,))
        o = DedupOpts(DEDUP_BOTH_STRANDS if both_strands is True else int(both_strands), kinds.get(bounds_kind, bounds_kind))
        n, tot, lev = C.c_uint64(), DedupTotal(), (C.c_uint64 * DEDUP_LEVELS)()
        cnt = WHOLE if count is None else int(count)
        own = out is None
        if own:
            have = int(self.parse_header(d_naf).n_sequences)
            rows = max(0, min(have - int(first), cnt)) if cnt != WHOLE else max(0, have - int(first))
            out = torch.empty(max(DEDUP_BYTES * rows, 1), dtype=torch.uint8, device=self.device)
        buf = None if out is False else out
        self._check(self.L.naf_gpu_unnaf_dedup(self.h, _ptr(d_naf), d_naf.numel(), C.byref(o), int(first), cnt, _ptr(bounds) if bounds is not None else None,
                                               _ptr(buf) if buf is not None else None, buf.numel() // DEDUP_BYTES if buf is not None else 0,
                                               C.byref(n), C.byref(tot), lev))
        levels = [int(v) for v in lev]
        if buf is None:
            return None, tot, levels
        view = buf[:DEDUP_BYTES * n.value]
        return (np.frombuffer(view.cpu().numpy().tobytes(), dtype=DEDUP_DTYPE) if own else view), tot, levels

    def unnaf_screen(self, d_naf, d_ref, k=27, min_hits=1, keep_matched=False, forward_only=False, bounds=None, bounds_kind="trim", first=0, count=None, out=None):
        """(rows, total): records [first, first + count) of the archive d_naf screened against the k-mers of ALL records of the archive d_ref
        (naf_gpu_unnaf_screen; both uint8 device tensors) -- k: 1 to 31; a read with min_hits or more k-mers in the reference's set is
        matched, and dropped unless keep_matched, which drops the others; forward_only: the k-mers as stored, not the smaller of a k-mer
        and its reverse complement; bounds: a uint8 device tensor of the rows unnaf_trim or unnaf_screen (bounds_kind "trim"), unnaf_clip
        ("clip") or unnaf_dedup ("dedup") wrote for the same records, whose (begin, end) are screened instead of the whole reads and whose
        rows without TRIM_KEPT take no part -- as a structured numpy array (SCREEN_DTYPE), one row per read, and a ScreenTotal.  out: a
        uint8 device tensor to take the table (40 bytes a row); then `rows` is the torch view of its first 40 * n bytes and too small a
        tensor raises NafGpuError(E_CAP).  out=False: the totals only."""
        import numpy as np
        import torch
        kinds = {"trim": SCREEN_BOUNDS_TRIM, "clip": SCREEN_BOUNDS_CLIP, "dedup": SCREEN_BOUNDS_DEDUP}
        if bounds_kind not in kinds and not isinstance(bounds_kind, int):
            raise ValueError("bounds_kind: 'trim', 'clip' or 'dedup', not %r" % (bounds_kind,))
        o = ScreenOpts(int(k), (SCREEN_KEEP_MATCHED if keep_matched else 0) | (SCREEN_FORWARD_ONLY if forward_only else 0), kinds.get(bounds_kind, bounds_kind), int(min_hits))
        n, tot = C.c_uint64(), ScreenTotal()
        cnt = WHOLE if count is None else int(count)
        own = out is None
        if own:
            have = int(self.parse_header(d_naf).n_sequences)
            rows = max(0, min(have - int(first), cnt)) if cnt != WHOLE else max(0, have - int(first))
            out = torch.empty(max(SCREEN_BYTES * rows, 1), dtype=torch.uint8, device=self.device)
        buf = None if out is False else out
        self._check(self.L.naf_gpu_unnaf_screen(self.h, _ptr(d_naf), d_naf.numel(), _ptr(d_ref), d_ref.numel(), C.byref(o), int(first), cnt,
                                                _ptr(bounds) if bounds is not None else None, _ptr(buf) if buf is not None else None,
                                                buf.numel() // SCREEN_BYTES if buf is not None else 0, C.byref(n), C.byref(tot)))
        if buf is None:
            return None, tot
        view = buf[:SCREEN_BYTES * n.value]
        return (np.frombuffer(view.cpu().numpy().tobytes(), dtype=SCREEN_DTYPE) if own else view), tot

    @staticmethod
    def _run_class(cls, each, masked):
        """(set, flags) of a runs call; cls: a class as text (parse_base_class) or as the 16-bit set; None with masked."""
        flags = (RUNS_EACH if each else 0) | (RUNS_MASKED if masked else 0)
        s = 0 if cls is None else parse_base_class(cls) if isinstance(cls, (str, bytes)) else int(cls)
        if not 0 <= s <= 0xFFFF:
            raise ValueError("not a base class: %r" % (cls,))
        return s, flags

    def unnaf_runs_count(self, d_naf, cls, each=False, masked=False, min_len=1, first=0, count=None):
        """(n_runs, n_bases) of the runs unnaf_runs lists (naf_gpu_unnaf_runs_count)."""
        s, flags = self._run_class(cls, each, masked)
        n, nb = C.c_uint64(), C.c_uint64()
        self._check(self.L.naf_gpu_unnaf_runs_count(self.h, _ptr(d_naf), d_naf.numel(), s, flags, int(min_len), int(first), WHOLE if count is None else int(count),
                                                    C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def unnaf_runs(self, d_naf, cls, each=False, masked=False, min_len=1, first=0, count=None, out=None):
        """(rows, n_bases): the runs of at least min_len bases of base class `cls` -- text as parse_base_class takes it, or the 16-bit set;
        each: every code of it a class of its own -- or, with masked (cls None or 0), the soft-masked intervals, in records
        [first, first + count), as a structured numpy array (RUN_DTYPE: record, begin, end, code, reserved) in ascending (record, begin),
        and the sum of their lengths.  out: a uint8 device tensor to take the table (32 bytes a run); then `rows` is the torch view of
        its first 32 * n bytes and too small a tensor raises NafGpuError(E_CAP).  Without it a table sized by a guess is tried first and
        one of the whole count when that was too small (the call reports it with E_CAP)."""
        s, flags = self._run_class(cls, each, masked)
        n, nb = C.c_uint64(), C.c_uint64()
        cnt = WHOLE if count is None else int(count)

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_runs(self.h, _ptr(d_naf), d_naf.numel(), s, flags, int(min_len), int(first), cnt, _ptr(buf), cap, C.byref(n), C.byref(nb))
        rows = self._guessed_table(call, n, RUN_BYTES, RUN_DTYPE, out)
        return rows, nb.value

    @staticmethod
    def _repeat_spec(spec):
        """The RepeatSpec of a repeats call; spec: text (parse_repeat_spec) or a sequence of 16 numbers, [p - 1] the copies of period p."""
        vals = parse_repeat_spec(spec) if isinstance(spec, (str, bytes)) else [int(v) for v in spec]
        if len(vals) != 16 or not all(0 <= v < 2 ** 32 for v in vals):
            raise ValueError("not a repeat spec: %r" % (spec,))
        return RepeatSpec((C.c_uint32 * 16)(*vals))

    def unnaf_repeats_count(self, d_naf, spec="misa", min_len=1, whole_units=False, first=0, count=None):
        """(n_repeats, n_bases, per_period) of the rows unnaf_repeats lists (naf_gpu_unnaf_repeats_count); per_period: the sixteen counts,
        [p - 1] for period p."""
        sp = self._repeat_spec(spec)
        n, nb, pp = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 16)()
        self._check(self.L.naf_gpu_unnaf_repeats_count(self.h, _ptr(d_naf), d_naf.numel(), C.byref(sp), REPEATS_WHOLE_UNITS if whole_units else 0, int(min_len), int(first),
                                                       WHOLE if count is None else int(count), C.byref(n), C.byref(nb), pp))
        return n.value, nb.value, [int(v) for v in pp]

    def unnaf_repeats(self, d_naf, spec="misa", min_len=1, whole_units=False, first=0, count=None, out=None):
        """(rows, n_bases, per_period): the perfect tandem repeats of records [first, first + count) -- spec: MISA's definition syntax
        ("1-10,2-6,3-5", or "misa") or 16 numbers, the copies a repeat of period 1 .. 16 needs, 0: not searched; min_len: the bases a
        repeat needs; whole_units: a row's end is cut to a whole number of copies -- as a structured numpy array (REPEAT_DTYPE: record,
        begin, end, motif, period, reserved) in ascending (record, begin, period), the sum of their lengths and the rows per period.
        out: a uint8 device tensor to take the table (32 bytes a row); then `rows` is the torch view of its first 32 * n bytes and too
        small a tensor raises NafGpuError(E_CAP).  Without it a table sized by a guess is tried first and one of the whole count when
        that was too small (the call reports it with E_CAP)."""
        sp = self._repeat_spec(spec)
        n, nb, pp = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 16)()
        cnt, flags = WHOLE if count is None else int(count), REPEATS_WHOLE_UNITS if whole_units else 0

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_repeats(self.h, _ptr(d_naf), d_naf.numel(), C.byref(sp), flags, int(min_len), int(first), cnt, _ptr(buf), cap, C.byref(n), C.byref(nb), pp)
        rows = self._guessed_table(call, n, REPEAT_BYTES, REPEAT_DTYPE, out)
        return rows, nb.value, [int(v) for v in pp]

    @staticmethod
    def _orf_args(stops, starts, strands, split_unknown, closed):
        """(stops, starts, strands, flags) of an ORF call; the codon sets as text (parse_codon_set) or as 64-bit sets, starts None or 0:
        stop to stop."""
        st = parse_codon_set(stops) if isinstance(stops, (str, bytes)) else int(stops)
        sa = 0 if starts is None else parse_codon_set(starts) if isinstance(starts, (str, bytes)) else int(starts)
        if not (0 <= st < 2 ** 64 and 0 <= sa < 2 ** 64):
            raise ValueError("not a codon set: %r %r" % (stops, starts))
        return st, sa, int(strands), (ORF_SPLIT_UNKNOWN if split_unknown else 0) | (ORF_CLOSED if closed else 0)

    def unnaf_orfs_count(self, d_naf, stops="TAA,TAG,TGA", starts="ATG", min_len=75, strands=STRAND_BOTH, split_unknown=False, closed=False, first=0, count=None):
        """(n_orfs, n_bases, per_frame) of the rows unnaf_orfs lists (naf_gpu_unnaf_orfs_count); per_frame: the six counts [3 * strand + frame]."""
        st, sa, sd, flags = self._orf_args(stops, starts, strands, split_unknown, closed)
        n, nb, pf = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 6)()
        self._check(self.L.naf_gpu_unnaf_orfs_count(self.h, _ptr(d_naf), d_naf.numel(), st, sa, int(min_len), sd, flags, int(first), WHOLE if count is None else int(count),
                                                    C.byref(n), C.byref(nb), pf))
        return n.value, nb.value, [int(v) for v in pf]

    def unnaf_orfs(self, d_naf, stops="TAA,TAG,TGA", starts="ATG", min_len=75, strands=STRAND_BOTH, split_unknown=False, closed=False, first=0, count=None, out=None):
        """(rows, n_bases): the open reading frames of at least min_len bases on the strands asked for (STRAND_FORWARD, STRAND_REVERSE,
        STRAND_BOTH) of records [first, first + count) -- stops, starts: codon sets as text (parse_codon_set) or as 64-bit sets; starts
        None or 0: from stop to stop; split_unknown: a codon with N or another ambiguity code ends a reading frame; closed: only those
        that end in a stop -- as a structured numpy array (ORF_DTYPE: record, begin, end, strand, frame, flags) in ascending (record,
        begin, end, strand), and the sum of their lengths.  out: a uint8 device tensor to take the table (32 bytes a row); then `rows`
        is the torch view of its first 32 * n bytes and too small a tensor raises NafGpuError(E_CAP).  Without it a table sized by a
        guess is tried first and one of the whole count when that was too small (the call reports it with E_CAP)."""
        st, sa, sd, flags = self._orf_args(stops, starts, strands, split_unknown, closed)
        n, nb = C.c_uint64(), C.c_uint64()
        cnt = WHOLE if count is None else int(count)

        def call(buf, cap):
            return self.L.naf_gpu_unnaf_orfs(self.h, _ptr(d_naf), d_naf.numel(), st, sa, int(min_len), sd, flags, int(first), cnt, _ptr(buf), cap, C.byref(n), C.byref(nb))
        rows = self._guessed_table(call, n, ORF_BYTES, ORF_DTYPE, out)
        return rows, nb.value

    def unnaf_kmers_rows(self, d_naf, k, canonical=False, per_record=False, first=0, count=None):
        """(n_rows, n_counters) of the tables unnaf_kmers gives for records [first, first + count) (naf_gpu_unnaf_kmers_rows: the lengths
        only, no sequence is decoded)."""
        flags = (KMER_CANONICAL if canonical else 0) | (KMER_PER_RECORD if per_record else 0)
        n, nc = C.c_uint64(), C.c_uint64()
        self._check(self.L.naf_gpu_unnaf_kmers_rows(self.h, _ptr(d_naf), d_naf.numel(), int(k), flags, int(first), WHOLE if count is None else int(count),
                                                    C.byref(n), C.byref(nc)))
        return n.value, nc.value

    def unnaf_kmers(self, d_naf, k, canonical=False, per_record=False, first=0, count=None, out=None, out_rows=None):
        """(counts, rows, total): the exact counts of all 4**k k-mers (k = 1..12) of records [first, first + count) -- one table for the
        selection or, with per_record, one per record -- as a device torch.int64 tensor of shape (n_rows, 4**k); the rows (KMER_DTYPE:
        record, begin, end, positions, counted) as a structured numpy array, None without per_record; and their sum as a KmerRow (its
        record: the records covered, its end: their bases).  canonical: a k-mer and its reverse complement share the smaller index.
        out: a device torch.int64 tensor to take the tables; `counts` is then a view of it, and too small a tensor raises
        NafGpuError(E_CAP).  out_rows: a uint8 device tensor to take the rows (40 bytes a row); `rows` is then the torch view of the bytes
        written.  Without them the sizes are asked for first (naf_gpu_unnaf_kmers_rows)."""
        import numpy as np
        import torch
        flags = (KMER_CANONICAL if canonical else 0) | (KMER_PER_RECORD if per_record else 0)
        cnt = WHOLE if count is None else int(count)
        n, nc, tot = C.c_uint64(), C.c_uint64(), KmerRow()
        if out is None or (per_record and out_rows is None):
            self._check(self.L.naf_gpu_unnaf_kmers_rows(self.h, _ptr(d_naf), d_naf.numel(), int(k), flags, int(first), cnt, C.byref(n), C.byref(nc)))
        if out is None:
            buf = torch.empty(max(nc.value, 1), dtype=torch.int64, device=self.device)
        else:
            if out.dtype != torch.int64 or not out.is_contiguous():
                raise ValueError("out: a contiguous torch.int64 tensor")
            buf = out.view(-1)
        rows_buf = None
        if per_record:
            rows_buf = out_rows if out_rows is not None else torch.empty(max(KMER_ROW_BYTES * n.value, 1), dtype=torch.uint8, device=self.device)
        self._check(self.L.naf_gpu_unnaf_kmers(self.h, _ptr(d_naf), d_naf.numel(), int(k), flags, int(first), cnt, _ptr(buf), buf.numel(),
                                               _ptr(rows_buf) if rows_buf is not None else None, rows_buf.numel() // KMER_ROW_BYTES if rows_buf is not None else 0,
                                               C.byref(n), C.byref(nc), C.byref(tot)))
        counts = buf[:nc.value].view(n.value, 4 ** int(k))
        rows = None
        if per_record:
            view = rows_buf[:KMER_ROW_BYTES * n.value]
            rows = view if out_rows is not None else np.frombuffer(view.cpu().numpy().tobytes(), dtype=KMER_DTYPE)
        return counts, rows, tot

    def histogram(self, d_buf):
        """Byte counts of a device buffer (unnaf --charcount)."""
        cnt = (C.c_uint64 * 256)()
        self._check(self.L.naf_gpu_histogram(self.h, _ptr(d_buf), d_buf.numel(), cnt))
        return list(cnt)

    # ---- ennaf ----
    def ennaf(self, d_text, seq_type=SEQ_DNA, fmt=FMT_AUTO, no_mask=False, level=1, line_length=-1, title=None, out=None, strict=False, long_log=0):
        import torch
        o = EnnafOpts(fmt, seq_type, int(no_mask), int(strict), level, line_length, title, long_log)
        if out is None:
            cap = self.L.naf_gpu_ennaf_bound(d_text.numel())
            out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        n = C.c_size_t()
        rep = EnnafReport()
        self._check(self.L.naf_gpu_ennaf(self.h, _ptr(d_text), d_text.numel(), C.byref(o), _ptr(out), out.numel(), C.byref(n), C.byref(rep)))
        return out[:n.value], rep

    # ---- ennaf of one input on several GPUs: the per-shard calls (orchestration in naf_amd/shard.py) ----
    def ennaf_sniff(self, d_text, fmt=FMT_AUTO):
        f, p0 = C.c_int(), C.c_uint64()
        self._check(self.L.naf_gpu_ennaf_sniff(self.h, _ptr(d_text), d_text.numel(), fmt, C.byref(f), C.byref(p0)))
        return f.value, p0.value

    def ennaf_count_lines(self, d_slice, prev_is_eol):
        n = C.c_uint64()
        self._check(self.L.naf_gpu_ennaf_count_lines(self.h, _ptr(d_slice), d_slice.numel(), int(prev_is_eol), C.byref(n)))
        return n.value

    def ennaf_find_cut(self, d_slice, fmt, prev_is_eol, skip_lines=0):
        off = C.c_uint64()
        self._check(self.L.naf_gpu_ennaf_find_cut(self.h, _ptr(d_slice), d_slice.numel(), fmt, int(prev_is_eol), skip_lines, C.byref(off)))
        return off.value

    def ennaf_shard_begin(self, d_slice, opts, fmt, shard, n_shards):
        info = ShardInfo()
        self._check(self.L.naf_gpu_ennaf_shard_begin(self.h, _ptr(d_slice), d_slice.numel(), C.byref(opts), fmt, shard, n_shards, C.byref(info)))
        return info

    def ennaf_shard_finish(self, opts, infos, text_len):
        import torch
        cap = self.L.naf_gpu_ennaf_shard_bound(text_len)
        buf = torch.empty(cap, dtype=torch.uint8, device=self.device)
        arr = (ShardInfo * len(infos))(*infos)
        pc = ShardPieces()
        self._check(self.L.naf_gpu_ennaf_shard_finish(self.h, C.byref(opts), arr, _ptr(buf), cap, C.byref(pc)))
        return buf, pc

    def ennaf_stitch(self, segs, lit, bufs, out):
        sa = (StitchSeg * len(segs))(*segs)
        pa = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        self._check(self.L.naf_gpu_ennaf_stitch(self.h, sa, len(segs), lit, pa, _ptr(out), out.numel()))

    # ---- timing ----
    def set_timing(self, on):
        self._check(self.L.naf_gpu_set_timing(self.h, int(on)))

    def get_timing(self):
        cap = 160
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        cnt = (C.c_int * cap)()
        n = self.L.naf_gpu_get_timing(self.h, names, ms, cnt, cap)
        return [(names[i].decode(), ms[i], cnt[i]) for i in range(n)]

    def get_timing_streams(self):
        """Kernel time of the last get_timing() per stream: [caller's stream, side chain 1..4]."""
        ms = (C.c_float * 5)()
        self._check(self.L.naf_gpu_get_timing_streams(self.h, ms))
        return [float(x) for x in ms]

    def synchronize(self):
        self._check(self.L.naf_gpu_synchronize(self.h))
