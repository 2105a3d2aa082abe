/* unnaf -- NAF decompressor front end for the MI355X path.
 * Command line, outputs and messages follow unnaf/src/unnaf.c:197-456 and unnaf/src/output.c of the
 * reference; every decompression and the text re-emit run on the GPU through libnaf_gpu.so. */
#include "host_common.h"
#include <sys/mman.h>

typedef enum { UNDECIDED, FORMAT_NAME, PART_LIST, PART_SIZES, NUMBER_OF_SEQUENCES, TITLE, IDS, NAMES, LENGTHS, TOTAL_LENGTH,
               MASK, TOTAL_MASK_LENGTH, FOUR_BIT, DNA, MASKED_DNA, UNMASKED_DNA, SEQ, SEQUENCES, CHARCOUNT,
               FASTA, MASKED_FASTA, UNMASKED_FASTA, FASTQ } OUTPUT_TYPE;
static OUTPUT_TYPE out_type = UNDECIDED;
static bool use_mask = true, force_stdout = false, verbose = false;
static char *in_file_path = NULL, *out_file_path = NULL;
static bool line_length_is_specified = false; static long long requested_line_length = 0;
static FILE *OUT = NULL; static bool created_output_file = false, success = false;
/* --region / --rc-region / --records, in command-line order (this implementation only: the reference has no selection) */
typedef struct { const char *region; unsigned long long first, last; bool rc; } selection;      /* region, or records first..last (1-based, inclusive); rc: its reverse complement */
static selection *selections = NULL; static size_t n_selections = 0;
static bool revcomp = false;                                      /* --revcomp: every selection of the call as its reverse complement */
/* --locate PATTERN (up to 16) / --strand: where IUPAC motifs lie, as BED6 (this implementation only) */
enum { MAX_LOCATE = 16 };
static const char *locate_patterns[MAX_LOCATE]; static size_t n_locate = 0;
static int locate_strands = 3; static bool strand_given = false;
/* --mismatches N, or a pattern with [letters that must match]: the near search, BED6 with the count in column 5 and the site as a 7th column */
static unsigned locate_mismatches = 0; static bool mismatches_given = false, locate_bracketed = false;
static size_t locate_free_letters[MAX_LOCATE];                    /* a pattern's letters outside brackets */
/* --composition [--window N]: base composition per record or per window, as a tab-separated table (this implementation only) */
static bool composition = false, window_given = false; static unsigned long long comp_window = 0;
/* --quality [--cycles N]: quality statistics per read or per bin of N read positions, as a tab-separated table (this implementation only) */
static bool quality = false, cycles_given = false; static unsigned long long qual_cycles = 0;
/* --runs CLASS / --masked-runs [--min-run N] [--each]: runs of a base class or soft-masked intervals, as BED4 (this implementation only) */
static const char *runs_class = NULL; static uint16_t runs_set = 0; static bool masked_runs = false, runs_each = false, min_run_given = false;
static unsigned long long min_run = 1;
/* --kmers K [--canonical] [--per-record]: exact counts of all 4^K k-mers of the selection, or of every record (this implementation only) */
static unsigned kmers_k = 0; static bool kmers_canonical = false, kmers_per_record = false;
/* --orfs [--min-orf N] [--stops LIST] [--starts LIST | --stop-to-stop] [--strand +|-|both] [--closed] [--split-unknown]: open reading frames on
 * the six frames, one tab-separated line each (this implementation only) */
static bool orfs = false, min_orf_given = false, stop_to_stop = false, orfs_closed = false, orfs_split = false;
static const char *orf_stops_text = NULL, *orf_starts_text = NULL; static uint64_t orf_stops = 0, orf_starts = 0;
static unsigned long long min_orf = 75;
/* --repeats SPEC [--min-repeat N] [--whole-units]: perfect tandem repeats of period 1 to 16, as a table (this implementation only) */
static const char *repeats_text = NULL; static naf_gpu_repeat_spec repeats_spec; static bool min_repeat_given = false, whole_units = false;
static unsigned long long min_repeat = 1;
/* --translate [--frame LIST] [--code N | --code-table LETTERS64]: the selection's frames, or with --orfs every reading frame, as protein FASTA (this implementation only) */
static bool translate = false; static int frames[6] = { 1 }; static size_t n_frames = 1;
static const char *frame_text = NULL, *code_text = NULL, *code_table_text = NULL; static naf_gpu_genetic_code genetic_code;
/* --trim Q|none [--min-length N] [--max-ee X] [--trim-table]: the reads cut to their best stretch of quality codes and filtered, or the table of
 * the stretches (this implementation only) */
static const char *trim_text = NULL, *max_ee_text = NULL; static naf_gpu_trim_opts trim_opts = { 0, 1, UINT64_MAX };
static bool min_length_given = false, trim_table = false, reads_selection = false;      /* reads_selection: emit_segments writes reads (naf_gpu_unnaf_select_reads) */
/* --adapter SEQ (up to 16) [--adapter-errors R] [--min-overlap N] [--min-length N] [--clip-table] [--trim Q|none [--max-ee X]]: the reads cut where
 * a 3' adapter begins, behind the quality trimming when there is one, or the table of the clip points (this implementation only) */
static const char *adapters[NAF_GPU_CLIP_MAX_ADAPTERS]; static size_t n_adapters = 0;
static const char *adapter_errors_text = NULL; static unsigned long long adapter_num = 1, adapter_den = 10;
static naf_gpu_clip_opts clip_opts = { 3, 1 }; static bool min_overlap_given = false, clip_table = false;
/* --dedup [--either-strand] [--dedup-table] [--trim Q|none ...] [--adapter SEQ ...]: every distinct read once -- the first of its copies --, behind
 * the quality trimming and the adapter clipping when there are any, or the table of the classes (this implementation only) */
static bool dedup = false, either_strand = false, dedup_table = false;
/* --screen REF.naf [--screen-k K] [--min-hits N] [--keep-matched] [--forward-only] [--screen-table] [--trim ...] [--adapter ...] [--dedup ...]: the reads
 * that share no k-mer with the archive REF.naf (with --keep-matched: those that do), behind the quality trimming and the adapter clipping and in
 * front of the duplicate collapsing when there are any, or the table of the hits (this implementation only) */
static const char *screen_ref = NULL; static naf_gpu_screen_opts screen_opts = { 27, 0, 0, 1 };
static bool screen_k_given = false, min_hits_given = false, keep_matched = false, forward_only = false, screen_table = false;

static void done(int status, void *arg)
{
    (void)arg;
    if (!success && created_output_file && out_file_path) remove(out_file_path);
    trace_out();
    detach_report(status);                                        /* the foreground process leaves with this status now; what follows is nobody's wait */
    if (gpu_init_started) { pthread_join(gpu_init_thread, NULL); gpu_init_started = false; }       /* (an exit while the device is still being opened) */
    if (gpu) naf_gpu_shutdown(gpu);
}
static void set_out_type(OUTPUT_TYPE t) { if (out_type != UNDECIDED) die("only one output type should be specified\n"); out_type = t; }

static void set_line_length(char *str)
{
    long long a; int how = decimal_arg(str, &a);
    if (how == 0) die("can't parse the value of --line-length parameter\n");
    if (a < 0) die("negative line length specified\n");
    if (how != 2) die("can't parse the value of --line-length parameter\n");
    requested_line_length = a; line_length_is_specified = true;
}

static void add_selection(const char *region, unsigned long long first, unsigned long long last, bool rc)
{
    selections = (selection *)realloc(selections, (n_selections + 1) * sizeof *selections);
    if (!selections) die("can't allocate memory\n");
    selections[n_selections++] = (selection){ region, first, last, rc };
}
static void add_region(const char *spec, bool rc)
{
    size_t id_len; uint64_t b, e;
    if (naf_gpu_parse_region(spec, &id_len, &b, &e)) die("can't parse the value of %s parameter\n", rc ? "--rc-region" : "--region");
    add_selection(spec, 0, 0, rc);
}
static void add_records(const char *spec)
{
    char *end = NULL;
    if (*spec < '0' || *spec > '9') die("can't parse the value of --records parameter\n");
    unsigned long long a = strtoull(spec, &end, 10), b = a;
    if (*end == '-') { const char *q = end + 1; if (*q < '0' || *q > '9') die("can't parse the value of --records parameter\n"); b = strtoull(q, &end, 10); }
    if (*end || a == 0 || b < a) die("can't parse the value of --records parameter\n");
    add_selection(NULL, a, b, false);
}

static void add_locate(const char *pattern)
{
    uint8_t fwd[32], rev[32]; size_t len; uint32_t fixed;
    if (naf_gpu_compile_motif_near(pattern, fwd, rev, &fixed, &len))            /* (a pattern without brackets: the message it always had) */
        die(strpbrk(pattern, "[]") ? "can't parse the value of --locate parameter (1 to 32 IUPAC nucleotide letters, [] around those that must match)\n"
                                   : "can't parse the value of --locate parameter (1 to 32 IUPAC nucleotide letters)\n");
    if (n_locate == MAX_LOCATE) die("at most %d --locate patterns can be searched at once\n", (int)MAX_LOCATE);
    if (strchr(pattern, '[')) locate_bracketed = true;
    locate_free_letters[n_locate] = len - (size_t)__builtin_popcount(fixed);
    locate_patterns[n_locate++] = pattern;
}
static void set_mismatches(const char *v)
{
    if (mismatches_given) die("only one --mismatches value can be given\n");
    if (!(v[0] >= '0' && v[0] <= '0' + NAF_GPU_LOCATE_MAX_MISMATCHES && !v[1])) die("can't parse the value of --mismatches parameter (0 to %d)\n", NAF_GPU_LOCATE_MAX_MISMATCHES);
    locate_mismatches = (unsigned)(v[0] - '0'); mismatches_given = true;
}
static void set_strand(const char *v)
{
    if (!strcmp(v, "+")) locate_strands = 1; else if (!strcmp(v, "-")) locate_strands = 2; else if (!strcmp(v, "both")) locate_strands = 3;
    else die("can't parse the value of --strand parameter (+, - or both)\n");
    strand_given = true;
}

/* the n bytes at v as a number: digits, commas are skipped (1,000); false: not one, or too large */
static bool number_of(const char *v, size_t n, unsigned long long *out)
{
    unsigned long long a = 0; bool ok = false;
    for (const char *p = v; p < v + n; p++) {
        if (*p == ',') continue;
        ok = *p >= '0' && *p <= '9' && a <= (ULLONG_MAX - (unsigned)(*p - '0')) / 10;
        if (!ok) break;
        a = a * 10 + (unsigned)(*p - '0');
    }
    *out = a;
    return ok;
}
/* --window, --cycles, --min-run, --min-orf, --min-repeat, --min-length: a positive number of `unit` */
static unsigned long long positive_number(const char *opt, const char *unit, const char *v)
{
    unsigned long long a = 0;
    if (!number_of(v, strlen(v), &a) || a == 0) die("can't parse the value of %s parameter (a positive number of %s)\n", opt, unit);
    return a;
}

static void set_trim(const char *v)
{
    if (trim_text) die("only one --trim cutoff can be given\n");
    unsigned long long q = 0;
    if (!strcmp(v, "none")) trim_opts.limit = NAF_GPU_TRIM_NONE;
    else if (strchr(v, ',') || !number_of(v, strlen(v), &q) || q > 93 || naf_gpu_trim_limit((unsigned)q, &trim_opts.limit))
        die("can't parse the value of --trim parameter (a Phred score of 0 to 93, or none)\n");
    trim_text = v;
}
/* --max-ee X: digits, or digits '.' and 1 to 9 digits; floor(X * 2^32) in integers */
static void set_max_ee(const char *v)
{
    if (max_ee_text) die("only one --max-ee value can be given\n");
    const char *dot = strchr(v, '.');
    const size_t nw = dot ? (size_t)(dot - v) : strlen(v), nf = dot ? strlen(dot + 1) : 0;
    unsigned long long whole = 0, frac = 0, pow10 = 1;
    bool ok = !strchr(v, ',') && number_of(v, nw, &whole) && whole <= 0xFFFFFFFFull && (!dot || (nf >= 1 && nf <= 9 && number_of(dot + 1, nf, &frac)));
    if (!ok) die("can't parse the value of --max-ee parameter (expected errors: digits, or digits.digits with 1 to 9 behind the point)\n");
    for (size_t k = 0; k < nf; k++) pow10 *= 10;
    trim_opts.max_ee = (whole << 32) + (frac << 32) / pow10;                   /* frac < 10^9 < 2^30: no overflow */
    max_ee_text = v;
}

static void add_adapter(const char *v)
{
    uint8_t fwd[32], rev[32]; size_t len;
    if (strlen(v) > 32) die("--adapter %s has more than 32 letters: of a 3' adapter the first 32 decide the same clip points, give those\n", v);
    if (naf_gpu_compile_motif(v, fwd, rev, &len)) die("can't parse the value of --adapter parameter (1 to 32 IUPAC nucleotide letters)\n");
    if (n_adapters == NAF_GPU_CLIP_MAX_ADAPTERS) die("at most %d --adapter sequences can be clipped at once\n", (int)NAF_GPU_CLIP_MAX_ADAPTERS);
    adapters[n_adapters++] = v;
}
/* --adapter-errors R: 0, or 0.digits with 1 to 9 behind the point; kept as num / den */
static void set_adapter_errors(const char *v)
{
    if (adapter_errors_text) die("only one --adapter-errors value can be given\n");
    const char *dot = strchr(v, '.');
    const size_t nw = dot ? (size_t)(dot - v) : strlen(v), nf = dot ? strlen(dot + 1) : 0;
    unsigned long long whole = 0, frac = 0, pow10 = 1;
    bool ok = !strchr(v, ',') && number_of(v, nw, &whole) && whole == 0 && (!dot || (nf >= 1 && nf <= 9 && number_of(dot + 1, nf, &frac)));
    if (!ok) die("can't parse the value of --adapter-errors parameter (mismatches per overlapped letter, below 1: 0, or 0.digits with 1 to 9 behind the point)\n");
    for (size_t k = 0; k < nf; k++) pow10 *= 10;
    adapter_num = frac; adapter_den = pow10;
    adapter_errors_text = v;
}
static void set_min_overlap(const char *v)
{
    const unsigned long long a = positive_number("--min-overlap", "adapter letters", v);
    if (a > 32) die("can't parse the value of --min-overlap parameter (1 to 32 adapter letters)\n");
    clip_opts.min_overlap = (uint32_t)a; min_overlap_given = true;
}

static void set_runs(const char *v)
{
    if (runs_class) die("only one --runs class can be listed at a time\n");
    if (naf_gpu_parse_base_class(v, &runs_set) || !runs_set) die("can't parse the value of --runs parameter (letters of ACGTU RYSWKM BDHV N and -, ^ in front for all the others)\n");
    runs_class = v;
}

static void set_repeats(const char *v)
{
    if (repeats_text) die("only one --repeats definition can be given\n");
    if (naf_gpu_parse_repeat_spec(v, &repeats_spec)) die("can't parse the value of --repeats parameter (PERIOD-COPIES pairs joined by commas, periods 1 to 16, at least 2 copies, e.g. 1-10,2-6,3-5; or misa)\n");
    repeats_text = v;
}

static void set_screen(const char *v)
{
    if (screen_ref) die("only one --screen reference can be given\n");
    if (!*v) die("empty --screen parameter\n");
    screen_ref = v;
}
static void set_screen_k(const char *v)
{
    unsigned long long a = 0;
    if (!number_of(v, strlen(v), &a) || a < 1 || a > 31) die("can't parse the value of --screen-k parameter (a k-mer length of 1 to 31)\n");
    screen_opts.k = (uint32_t)a; screen_k_given = true;
}

static void set_kmers(const char *v)
{
    if (kmers_k) die("only one --kmers length can be counted at a time\n");
    unsigned a = 0; bool digit = false;
    for (const char *p = v; *p; p++) {
        if (*p < '0' || *p > '9' || a > 12) die("can't parse the value of --kmers parameter (a k-mer length of 1 to 12)\n");
        a = a * 10 + (unsigned)(*p - '0'); digit = true;
    }
    if (!digit || a < 1 || a > 12) die("can't parse the value of --kmers parameter (a k-mer length of 1 to 12)\n");
    kmers_k = a;
}

static void set_codons(const char *opt, const char *v, const char **text, uint64_t *set)
{
    if (*text) die("only one %s list can be given\n", opt);
    if (naf_gpu_parse_codon_set(v, set)) die("can't parse the value of %s parameter (comma-separated codons of three IUPAC nucleotide letters, e.g. TAA,TAG,TGA)\n", opt);
    *text = v;
}

static void set_frames(const char *v)
{
    if (frame_text) die("only one --frame list can be given\n");
    frame_text = v; n_frames = 0;
    if (!strcmp(v, "6")) { static const int all[6] = { 1, 2, 3, -1, -2, -3 }; memcpy(frames, all, sizeof all); n_frames = 6; return; }
    for (const char *p = v; ; p++) {
        const bool minus = *p == '-'; if (minus) p++;
        if (*p < '1' || *p > '3' || (p[1] && p[1] != ',') || n_frames == 6) die("can't parse the value of --frame parameter (comma-separated frames out of 1,2,3,-1,-2,-3, or 6 for all six)\n");
        const int f = minus ? -(*p - '0') : *p - '0';
        for (size_t k = 0; k < n_frames; k++) if (frames[k] == f) die("can't parse the value of --frame parameter (comma-separated frames out of 1,2,3,-1,-2,-3, or 6 for all six)\n");
        frames[n_frames++] = f;
        if (!*++p) break;
    }
}
static void set_code(const char *v)
{
    if (code_text) die("only one --code can be given\n");
    int id = 0; bool ok = *v != 0;
    for (const char *p = v; *p && ok; p++) { ok = *p >= '0' && *p <= '9' && id < 100; id = id * 10 + (*p - '0'); }
    if (!ok || naf_gpu_genetic_code_by_id(id, &genetic_code)) die("can't parse the value of --code parameter (the number of an NCBI genetic code: 1 to 6, 9 to 16, 21 to 26)\n");
    code_text = v;
}
static void set_code_table(const char *v)
{
    if (code_table_text) die("only one --code-table can be given\n");
    naf_gpu_genetic_code g;
    if (naf_gpu_genetic_code_parse(v, &g)) die("can't parse the value of --code-table parameter (64 letters A to Z or *, the codons in the order AAA AAC AAG AAT ACA ... TTT)\n");
    code_table_text = v;
    if (!code_text) genetic_code = g;                                /* (both given is refused later) */
}

static void show_help(void)
{
    msg("Usage: unnaf [OUTPUT-TYPE] [file.naf]\n"
        "Options for selecting output type:\n"
        "  --format        - File format version\n  --part-list     - List of parts\n  --sizes         - Part sizes\n"
        "  --number        - Number of sequences\n  --title         - Dataset title\n  --ids           - Sequence ids (accession numbers)\n"
        "  --names         - Full sequence names (including ids)\n  --lengths       - Sequence lengths\n  --total-length  - Sum of sequence lengths\n"
        "  --mask          - Masked region lengths\n  --4bit          - 4bit-encoded nucleotide sequence (binary data)\n"
        "  --seq           - Continuous concatenated sequence\n  --sequences     - One sequence per line, no names\n"
        "  --fasta         - FASTA-formatted sequences\n  --fastq         - FASTQ-formatted sequences\n"
        "Other options:\n  -o FILE         - Decompress into FILE\n  -c              - Write to standard output\n"
        "  --line-length N - Use lines of width N for FASTA output\n  --no-mask       - Ignore mask\n"
        "  --binary-stdout - Set stdout stream to binary mode.\n  --binary-stderr - Set stderr stream to binary mode.\n"
        "  --binary        - Shortcut for \"--binary-stdout --binary-stderr\"\n  -h, --help      - Show help\n  -V, --version   - Show version\n"
        "Options for selecting records (with --fasta, --fastq, --seq, --sequences; repeatable, output in the order given):\n"
        "  --region ID[:A-B] - Sequence ID, or its bases A to B (1-based, inclusive; \"ID:A-\" = to its end)\n"
        "  --records A-B   - Sequences number A to B (1-based, inclusive)\n"
        "  --rc-region ID[:A-B] - The same region as its reverse complement (header \"ID:A-B/rc\"; DNA and RNA only)\n"
        "  --revcomp       - Every selected sequence and region as its reverse complement\n"
        "Options for searching (output: BED6 lines \"ID begin end PATTERN 0 strand\", 0-based half-open; with at most one --records A-B or --region ID):\n"
        "  --locate PATTERN - Every place where the IUPAC pattern (1 to 32 letters, e.g. NGG) matches; repeatable, up to 16 patterns\n"
        "  --strand +|-|both - Search the sequences as stored, their reverse complement, or both (default)\n"
        "  --mismatches N  - With --locate: every place within N = 0 to 8 mismatches of a pattern; letters in [] must match, e.g. GAGTCCGAGCAGAAGAAGAA[NGG].\n"
        "                    With it, or with [] in a pattern, lines are \"ID begin end PATTERN mismatches strand SITE\": SITE is the pattern, mismatched letters in lower case\n"
        "Options for counting (output: a tab-separated table \"#seq start end A C G T N other gap masked CpG GC\"; with at most one --records A-B or --region ID):\n"
        "  --composition   - Base composition of every sequence: bases per letter, soft-masked bases, CpG, GC fraction (--no-mask: masked = 0)\n"
        "  --window N      - With --composition: one line per window of N bases instead of one per sequence\n"
        "  --quality       - Quality of every read, from the stored quality codes: \"#seq length mean min max q20 q30 ee\" (Phred+33; ee: expected errors)\n"
        "  --cycles N      - With --quality: one line per N read positions instead, over all reads: \"#cycle_begin cycle_end n mean min max q20 q30 ee\"\n"
        "Options for listing runs (output: BED4 lines \"ID begin end NAME\", 0-based half-open; with at most one --records A-B or --region ID):\n"
        "  --runs CLASS    - Every maximal run of bases of CLASS: letters of ACGTU RYSWKM BDHV N and -, taken literally (N is the stored N only); ^CLASS = all other codes\n"
        "  --masked-runs   - Every soft-masked interval (NAME is \"mask\")\n"
        "  --min-run N     - With --runs or --masked-runs: only runs of at least N bases (default 1)\n"
        "  --each          - With --runs: every letter of CLASS on its own, e.g. homopolymers for ACGT (NAME is the run's letter)\n"
        "Options for counting k-mers (output: lines \"KMER COUNT\" of the k-mers that occur, tab-separated; with at most one --records A-B or --region ID):\n"
        "  --kmers K       - Exact counts of all k-mers of K = 1 to 12 bases made of A, C, G, T/U only, never across a sequence's end; case is ignored\n"
        "  --canonical     - With --kmers: a k-mer and its reverse complement are counted as the one that sorts first\n"
        "  --per-record    - With --kmers, K up to 6: a table \"#seq length counted\" and one column per k-mer, one line per sequence\n"
        "Options for listing open reading frames (output: lines \"ID begin end FRAME CODONS STRAND stop|open\", tab-separated, 0-based half-open, the stop codon not included;\n"
        "    FRAME is +1..+3, or -1..-3 counted from the end of the sequence; with at most one --records A-B or --region ID):\n"
        "  --orfs          - Every open reading frame on the six frames of every sequence, from its first start codon to the stop; codons with N or another ambiguity code are no stops\n"
        "  --min-orf N     - With --orfs: only reading frames of at least N bases (default 75)\n"
        "  --stops LIST    - With --orfs: the stop codons, comma-separated, IUPAC letters allowed (default TAA,TAG,TGA)\n"
        "  --starts LIST   - With --orfs: the start codons (default ATG)\n"
        "  --stop-to-stop  - With --orfs: the whole stretch between two stops, whether it has a start codon or not\n"
        "  --closed        - With --orfs: only reading frames that end in a stop codon, none that run into the end of the sequence\n"
        "  --split-unknown - With --orfs: a codon with N or another ambiguity code ends a reading frame\n"
        "  --strand +|-|both - With --orfs: the sequences as stored, their reverse complement, or both (default)\n"
        "Options for translating (output: protein FASTA, headers as --region and --rc-region write them, stops as *, X for a codon that is not determined;\n"
        "    with any number of --records, --region, --rc-region; without one, every sequence):\n"
        "  --translate     - The amino acids of every selected sequence or region, read from its first base; one or two trailing bases are dropped.\n"
        "                    With --orfs: the protein of every reading frame of the table, in the table's order, instead of the table\n"
        "  --frame LIST    - With --translate: comma-separated frames out of 1,2,3,-1,-2,-3, or 6 for all six (default 1); -1..-3 count from the end, as in --orfs\n"
        "  --code N        - With --translate: NCBI genetic code N (1 to 6, 9 to 16, 21 to 26; default 1). With --orfs and without --stops, its stops close the reading frames\n"
        "  --code-table LETTERS - With --translate: a genetic code of its own, 64 letters A-Z or * for the codons AAA AAC AAG AAT ACA ... TTT\n"
        "  --repeats SPEC  - Every perfect tandem repeat, as lines \"ID begin end PERIOD MOTIF COPIES CLASS\" (0-based half-open): SPEC is PERIOD-COPIES pairs, e.g. 1-10,2-6,3-5, periods 1 to 16; or misa\n"
        "  --min-repeat N  - With --repeats: only repeats of at least N bases (default 1)\n"
        "  --whole-units   - With --repeats: the end of a repeat is cut to a whole number of copies, as MISA and PERF print it\n"
        "Options for screening reads against a reference (output: the reads that share no k-mer with it, as --fastq, --fasta, --sequences or --seq; with at most one --records A-B or --region ID):\n"
        "  --screen REF.naf - Drop every read that has a k-mer of the archive REF.naf (FASTA or FASTQ, DNA or RNA; make it with ennaf), on either strand; k-mers are made of A, C, G, T/U only\n"
        "                    and never run across a sequence's end. With --trim Q and / or --adapter SEQ the reads are trimmed and clipped first; with --dedup the kept reads are collapsed afterwards\n"
        "  --screen-k K    - With --screen: the k-mer length, 1 to 31 (default 27)\n"
        "  --min-hits N    - With --screen: a read matches when N of its k-mers are in the reference (default 1)\n"
        "  --keep-matched  - With --screen: keep the reads that match and drop the others\n"
        "  --forward-only  - With --screen: compare the k-mers as stored, not also their reverse complements\n"
        "  --screen-table  - With --screen: instead of the reads, a table \"#seq length begin end hits status\" of all reads (status clean, matched, or short / errors / duplicate)\n"
        "Options for collapsing duplicate reads (output: every distinct read once, the first of its copies, as --fastq, --fasta, --sequences or --seq; with at most one --records A-B or --region ID):\n"
        "  --dedup         - Drop every read whose bases are exactly those of an earlier read; case, qualities and names play no part, N equals only N.\n"
        "                    With --trim Q and / or --adapter SEQ the reads are trimmed and clipped first, and what is left of them is compared and written\n"
        "  --either-strand - With --dedup: a read that is the reverse complement of an earlier read is a copy of it too\n"
        "  --dedup-table   - With --dedup: instead of the reads, a table \"#seq length begin end first copies strand status\" of all reads (first: the read it copies; status first, duplicate, or short / errors)\n"
        "Options for clipping adapters (output: the kept reads, each cut where its 3' adapter begins, as --fastq, --fasta, --sequences or --seq; with at most one --records A-B or --region ID):\n"
        "  --adapter SEQ   - Cut every read at the leftmost place where SEQ (1 to 32 IUPAC letters) begins, also one that the read's end cuts short; repeatable, up to 16 adapters.\n"
        "                    With --trim Q (and --max-ee X) the reads are trimmed by quality first and the adapter is searched in what is left; --min-length N drops reads cut shorter than N\n"
        "  --adapter-errors R - With --adapter: floor(R * L) mismatches are allowed where L letters of the adapter lie in the read (default 0.1)\n"
        "  --min-overlap N - With --adapter: at least N letters of the adapter must lie in the read (default 3)\n"
        "  --clip-table    - With --adapter: instead of the reads, a table \"#seq length begin end adapter mismatches overlap status\" of all reads (adapter: its number from 1, or .)\n"
        "Options for trimming reads by quality (output: the kept reads, each cut to its stretch, as --fastq (default), --fasta, --sequences or --seq; with at most one --records A-B or --region ID):\n"
        "  --trim Q        - Of every read the stretch of the largest sum of (error rate of Phred Q) - (error rate of the code), Q = 0 to 93: the Phred / Mott rule of seqtk and BBDuk; none = the whole read\n"
        "  --min-length N  - With --trim: drop reads whose stretch has fewer than N bases (default 1)\n"
        "  --max-ee X      - With --trim: drop reads whose stretch has more than X expected errors, e.g. 2 or 0.5\n"
        "  --trim-table    - With --trim: instead of the reads, a table \"#seq length begin end ee status\" of all reads (0-based half-open; status kept, short, errors or short,errors)\n");
}

/* ---- the table modes ---------------------------------------------------------------------------------------------------------------
 * --locate, --composition, --quality, --runs / --masked-runs, --kmers, --orfs, --translate, --repeats, --screen, --dedup, --adapter and --trim write a table of their own
 * instead of an output type (--trim without --trim-table: the reads, in one of the sequence output types).  A mode is a row here -- what its refusals say, its options, its runner -- plus the checks that are
 * really its own; parse_command_line walks the rows once, in this order, and main runs the first one asked for (--orfs in front
 * of --translate: the one legal pair). */
typedef struct { bool given, fits; const char *refusal; } satellite;        /* an option of a mode: given; given together with what it belongs to */
typedef struct table_mode {
    bool asked; const char *name;                   /* the option, as messages name the mode */
    const char *writes;                             /* "NAME writes WRITES: no output type can be given with it" */
    const char *strands;                            /* "NAME STRANDS: --revcomp [--rc-region] can't be used with it" */
    bool one_selection;                             /* at most one --records or one --region ID, as stored (not --translate: any selection) */
    bool type_first;                                /* the output type is refused in front of another mode, not behind it */
    bool sequence_types;                            /* --fasta, --fastq, --seq and --sequences are its own output types: only the others are refused */
    satellite sat[7];                               /* refused without the mode, in this order; ends at the first without a refusal */
    void (*early)(void);                            /* what holds whether the mode was asked for or not, behind the satellites */
    void (*own)(const struct table_mode *);         /* the mode's own checks and defaults, behind the output type */
    const char *protein;                            /* main's refusal of protein and text archives (%s: which), NULL: none */
    void (*run)(bool has_ids, bool has_names);
} table_mode;
enum { M_LOCATE, M_COMPOSITION, M_QUALITY, M_RUNS, M_KMERS, M_ORFS, M_TRANSLATE, M_REPEATS, M_SCREEN, M_DEDUP, M_CLIP, M_TRIM, N_MODES };
static table_mode modes[N_MODES];
static void run_locate(bool, bool), run_composition(bool, bool), run_quality(bool, bool), run_runs(bool, bool), run_kmers(bool, bool), run_orfs(bool, bool),
            run_translate(bool, bool), run_repeats(bool, bool), run_screen(bool, bool), run_dedup(bool, bool), run_clip(bool, bool), run_trim(bool, bool);

static void refuse_output_type(const table_mode *m)
{
    if (m->sequence_types && (out_type == FASTA || out_type == FASTQ || out_type == SEQ || out_type == SEQUENCES)) return;
    if (out_type != UNDECIDED) die("%s writes %s: no %soutput type can be given with it\n", m->name, m->writes, m->sequence_types ? "other " : "");
}
static void refuse_revcomp(const table_mode *m) { if (revcomp) die("%s %s: --revcomp can't be used with it\n", m->name, m->strands); }
static void one_whole_selection(const table_mode *m)
{
    refuse_revcomp(m);
    if (n_selections > 1) die("%s can be restricted by one --records or one --region only\n", m->name);
    if (n_selections && selections[0].rc) die("%s %s: --rc-region can't be used with it\n", m->name, m->strands);
    if (n_selections && selections[0].region) {
        size_t l; uint64_t b, e; naf_gpu_parse_region(selections[0].region, &l, &b, &e);
        if (!(b == 0 && e == NAF_GPU_WHOLE)) die("%s can be restricted to a whole sequence only: --region ID, without a range\n", m->name);
    }
}

static void locate_early(void)
{
    if (locate_mismatches) for (size_t k = 0; k < n_locate; k++) if (locate_mismatches >= locate_free_letters[k])
        die("--mismatches %u leaves nothing of --locate %s to match: it must be smaller than the pattern's %zu letters outside brackets\n", locate_mismatches, locate_patterns[k], locate_free_letters[k]);
}
static void runs_early(void) { if (runs_class && masked_runs) die("--runs and --masked-runs can't be used together\n"); }
static void kmers_own(const table_mode *m)
{
    (void)m;
    if (kmers_per_record && kmers_k > 6) die("--per-record writes one column per k-mer: --kmers can be 6 at the most with it\n");
}
static void orfs_own(const table_mode *m)
{
    if (stop_to_stop && orf_starts_text) die("--stop-to-stop and --starts can't be used together\n");
    if (!orf_stops_text && translate && (code_text || code_table_text)) naf_gpu_genetic_code_stops(&genetic_code, &orf_stops);      /* the code's own stops close the frames */
    else if (!orf_stops_text) naf_gpu_parse_codon_set("TAA,TAG,TGA", &orf_stops);
    if (stop_to_stop) orf_starts = 0; else if (!orf_starts_text) naf_gpu_parse_codon_set("ATG", &orf_starts);
    if (orf_starts & orf_stops) die("--starts and --stops share a codon: a codon can't both open and close a reading frame\n");
    refuse_revcomp(m);                                              /* (in front of --frame, where it always stood) */
    if (frame_text && translate) die("--frame can't be used with --orfs: every reading frame of the table is translated in its own frame\n");
}
static void translate_own(const table_mode *m)
{
    (void)m;
    if (code_text && code_table_text) die("--code and --code-table can't be used together\n");
    if (!code_text && !code_table_text) naf_gpu_genetic_code_by_id(1, &genetic_code);
}

static void clip_own(const table_mode *m)
{
    (void)m;
    if (trim_table) die("--trim-table can't be used with --adapter: --clip-table writes the table of the clipped reads\n");
}

static void dedup_own(const table_mode *m)
{
    (void)m;
    if (trim_table) die("--trim-table can't be used with --dedup: --dedup-table writes the table of the collapsed reads\n");
    if (clip_table) die("--clip-table can't be used with --dedup: --dedup-table writes the table of the collapsed reads\n");
}

static void screen_own(const table_mode *m)
{
    (void)m;
    if (trim_table) die("--trim-table can't be used with --screen: --screen-table writes the table of the screened reads\n");
    if (clip_table) die("--clip-table can't be used with --screen: --screen-table writes the table of the screened reads\n");
    if (dedup_table) die("--dedup-table can't be used with --screen: --screen-table writes the table of the screened reads\n");
}

/* the rows, from the options as they were given */
static void fill_modes(void)
{
    const bool runs = runs_class || masked_runs;
    modes[M_LOCATE] = (table_mode){ .asked = n_locate != 0, .name = "--locate", .writes = "BED lines", .strands = "searches both strands itself (--strand)", .one_selection = true,
        .sat = { { strand_given, n_locate || orfs, "--strand can be used only with --locate\n" }, { mismatches_given, n_locate != 0, "--mismatches can be used only with --locate\n" } },
        .early = locate_early, .protein = "nucleotide motifs cannot be searched in %s sequences\n", .run = run_locate };
    modes[M_COMPOSITION] = (table_mode){ .asked = composition, .name = "--composition", .writes = "a table", .strands = "counts the sequences as stored", .one_selection = true,
        .sat = { { window_given, composition, "--window can be used only with --composition\n" } },
        .protein = "nucleotides cannot be counted in %s sequences\n", .run = run_composition };
    modes[M_QUALITY] = (table_mode){ .asked = quality, .name = "--quality", .writes = "a table", .strands = "reads the qualities as stored", .one_selection = true,
        .sat = { { cycles_given, quality, "--cycles can be used only with --quality\n" } }, .run = run_quality };
    modes[M_RUNS] = (table_mode){ .asked = runs, .name = runs_class ? "--runs" : "--masked-runs", .writes = "BED lines", .strands = "lists the sequences as stored", .one_selection = true,
        .sat = { { min_run_given, runs, "--min-run can be used only with --runs or --masked-runs\n" }, { runs_each, runs_class != NULL, "--each can be used only with --runs\n" } },
        .early = runs_early, .protein = "runs of bases cannot be listed in %s sequences\n", .run = run_runs };
    modes[M_KMERS] = (table_mode){ .asked = kmers_k != 0, .name = "--kmers", .writes = "a table", .strands = "counts the sequences as stored", .one_selection = true,
        .sat = { { kmers_canonical, kmers_k != 0, "--canonical can be used only with --kmers\n" }, { kmers_per_record, kmers_k != 0, "--per-record can be used only with --kmers\n" } },
        .own = kmers_own, .protein = "k-mers cannot be counted in %s sequences\n", .run = run_kmers };
    modes[M_ORFS] = (table_mode){ .asked = orfs, .name = "--orfs", .writes = "a table", .strands = "reads both strands itself (--strand)", .one_selection = true,
        .sat = { { min_orf_given, orfs, "--min-orf can be used only with --orfs\n" }, { orf_stops_text != NULL, orfs, "--stops can be used only with --orfs\n" },
                 { orf_starts_text != NULL, orfs, "--starts can be used only with --orfs\n" }, { stop_to_stop, orfs, "--stop-to-stop can be used only with --orfs\n" },
                 { orfs_closed, orfs, "--closed can be used only with --orfs\n" }, { orfs_split, orfs, "--split-unknown can be used only with --orfs\n" } },
        .own = orfs_own, .protein = "open reading frames cannot be listed in %s sequences\n", .run = run_orfs };
    modes[M_TRANSLATE] = (table_mode){ .asked = translate, .name = "--translate", .writes = "protein FASTA", .type_first = true,
        .sat = { { frame_text != NULL, translate, "--frame can be used only with --translate\n" }, { code_text != NULL, translate, "--code can be used only with --translate\n" },
                 { code_table_text != NULL, translate, "--code-table can be used only with --translate\n" } },
        .own = translate_own, .protein = "%s sequences cannot be translated\n", .run = run_translate };
    modes[M_REPEATS] = (table_mode){ .asked = repeats_text != NULL, .name = "--repeats", .writes = "a table", .strands = "lists the sequences as stored", .one_selection = true,
        .sat = { { min_repeat_given, repeats_text != NULL, "--min-repeat can be used only with --repeats\n" }, { whole_units, repeats_text != NULL, "--whole-units can be used only with --repeats\n" } },
        .protein = "tandem repeats cannot be listed in %s sequences\n", .run = run_repeats };
    /* --screen stands in front of --dedup, --adapter and --trim, the three modes it can be used with: main then runs it; it trims and clips first and collapses last */
    modes[M_SCREEN] = (table_mode){ .asked = screen_ref != NULL, .name = "--screen", .writes = screen_table ? "a table" : "reads as --fastq, --fasta, --sequences or --seq",
        .strands = "writes the reads as stored", .one_selection = true, .type_first = true, .sequence_types = !screen_table,
        .sat = { { screen_k_given, screen_ref != NULL, "--screen-k can be used only with --screen\n" }, { min_hits_given, screen_ref != NULL, "--min-hits can be used only with --screen\n" },
                 { keep_matched, screen_ref != NULL, "--keep-matched can be used only with --screen\n" }, { forward_only, screen_ref != NULL, "--forward-only can be used only with --screen\n" },
                 { screen_table, screen_ref != NULL, "--screen-table can be used only with --screen\n" } },
        .own = screen_own, .protein = "reads cannot be screened in %s sequences\n", .run = run_screen };
    /* --dedup stands in front of --adapter and --trim, the two modes it can be used with: main then runs it, and it trims and clips first */
    modes[M_DEDUP] = (table_mode){ .asked = dedup, .name = "--dedup", .writes = dedup_table ? "a table" : "reads as --fastq, --fasta, --sequences or --seq",
        .strands = "writes the reads as stored", .one_selection = true, .type_first = true, .sequence_types = !dedup_table,
        .sat = { { either_strand, dedup, "--either-strand can be used only with --dedup\n" }, { dedup_table, dedup, "--dedup-table can be used only with --dedup\n" } },
        .own = dedup_own, .protein = "duplicates cannot be collapsed in %s sequences\n", .run = run_dedup };
    /* --adapter stands in front of --trim, the one mode it can be used with: main then runs it, and it trims first */
    modes[M_CLIP] = (table_mode){ .asked = n_adapters != 0, .name = "--adapter", .writes = clip_table ? "a table" : "reads as --fastq, --fasta, --sequences or --seq",
        .strands = "clips the reads as stored", .one_selection = true, .type_first = true, .sequence_types = !clip_table,
        .sat = { { adapter_errors_text != NULL, n_adapters != 0, "--adapter-errors can be used only with --adapter\n" }, { min_overlap_given, n_adapters != 0, "--min-overlap can be used only with --adapter\n" },
                 { clip_table, n_adapters != 0, "--clip-table can be used only with --adapter\n" } },
        .own = clip_own, .protein = "adapters cannot be clipped in %s sequences\n", .run = run_clip };
    modes[M_TRIM] = (table_mode){ .asked = trim_text != NULL, .name = "--trim", .writes = trim_table ? "a table" : "reads as --fastq, --fasta, --sequences or --seq",
        .strands = "writes the reads as stored", .one_selection = true, .type_first = true, .sequence_types = !trim_table,
        .sat = { { min_length_given, trim_text != NULL || n_adapters != 0, "--min-length can be used only with --trim or --adapter\n" }, { max_ee_text != NULL, trim_text != NULL, "--max-ee can be used only with --trim\n" },
                 { trim_table, trim_text != NULL, "--trim-table can be used only with --trim\n" } },
        .run = run_trim };
}
static const table_mode *asked_mode(void)
{
    for (const table_mode *m = modes; m < modes + N_MODES; m++) if (m->asked) return m;
    return NULL;
}

static void parse_command_line(int argc, char **argv)
{
    bool print_version = false;
    static const struct { const char *name; OUTPUT_TYPE t; } types[] = {
        {"--format", FORMAT_NAME}, {"--part-list", PART_LIST}, {"--sizes", PART_SIZES}, {"--number", NUMBER_OF_SEQUENCES}, {"--title", TITLE},
        {"--ids", IDS}, {"--names", NAMES}, {"--lengths", LENGTHS}, {"--total-length", TOTAL_LENGTH}, {"--mask", MASK},
        {"--total-mask-length", TOTAL_MASK_LENGTH}, {"--4bit", FOUR_BIT}, {"--seq", SEQ}, {"--sequences", SEQUENCES}, {"--charcount", CHARCOUNT},
        {"--fasta", FASTA}, {"--fastq", FASTQ}, {"--dna", DNA}, {"--masked-dna", MASKED_DNA}, {"--unmasked-dna", UNMASKED_DNA},
        {"--masked-fasta", MASKED_FASTA}, {"--unmasked-fasta", UNMASKED_FASTA} };
    /* the other options (unnaf/src/unnaf.c:282-353), as a table: one that takes a value is only recognised with an argument behind it */
    enum { OP_LINE_LENGTH, OP_OUT, OP_NO_MASK, OP_IGNORED, OP_HELP, OP_VERBOSE, OP_VERSION, OP_STDOUT, OP_REGION, OP_RECORDS, OP_RC_REGION, OP_REVCOMP, OP_LOCATE, OP_STRAND, OP_MISMATCHES, OP_COMPOSITION, OP_WINDOW, OP_QUALITY, OP_CYCLES, OP_RUNS, OP_MASKED_RUNS, OP_MIN_RUN, OP_EACH, OP_KMERS, OP_CANONICAL, OP_PER_RECORD, OP_ORFS, OP_MIN_ORF, OP_STOPS, OP_STARTS, OP_STOP_TO_STOP, OP_CLOSED, OP_SPLIT_UNKNOWN, OP_TRANSLATE, OP_FRAME, OP_CODE, OP_CODE_TABLE, OP_REPEATS, OP_MIN_REPEAT, OP_WHOLE_UNITS, OP_TRIM, OP_MIN_LENGTH, OP_MAX_EE, OP_TRIM_TABLE, OP_ADAPTER, OP_ADAPTER_ERRORS, OP_MIN_OVERLAP, OP_CLIP_TABLE, OP_DEDUP, OP_EITHER_STRAND, OP_DEDUP_TABLE, OP_SCREEN, OP_SCREEN_K, OP_MIN_HITS, OP_KEEP_MATCHED, OP_FORWARD_ONLY, OP_SCREEN_TABLE };
    static const struct { const char *name; int op; bool value; } option_table[] = {
        { "--line-length", OP_LINE_LENGTH, true }, { "-o", OP_OUT, true }, { "--no-mask", OP_NO_MASK, false }, { "--binary-stdout", OP_IGNORED, false },
        { "--binary-stderr", OP_IGNORED, false }, { "--binary", OP_IGNORED, false }, { "--help", OP_HELP, false }, { "-h", OP_HELP, false },
        { "--verbose", OP_VERBOSE, false }, { "--version", OP_VERSION, false }, { "-V", OP_VERSION, false }, { "-c", OP_STDOUT, false },
        { "--region", OP_REGION, true }, { "--records", OP_RECORDS, true }, { "--rc-region", OP_RC_REGION, true }, { "--revcomp", OP_REVCOMP, false },
        { "--locate", OP_LOCATE, true }, { "--strand", OP_STRAND, true }, { "--mismatches", OP_MISMATCHES, true }, { "--composition", OP_COMPOSITION, false }, { "--window", OP_WINDOW, true },
        { "--quality", OP_QUALITY, false }, { "--cycles", OP_CYCLES, true },
        { "--runs", OP_RUNS, true }, { "--masked-runs", OP_MASKED_RUNS, false }, { "--min-run", OP_MIN_RUN, true }, { "--each", OP_EACH, false },
        { "--kmers", OP_KMERS, true }, { "--canonical", OP_CANONICAL, false }, { "--per-record", OP_PER_RECORD, false },
        { "--orfs", OP_ORFS, false }, { "--min-orf", OP_MIN_ORF, true }, { "--stops", OP_STOPS, true }, { "--starts", OP_STARTS, true }, { "--stop-to-stop", OP_STOP_TO_STOP, false },
        { "--closed", OP_CLOSED, false }, { "--split-unknown", OP_SPLIT_UNKNOWN, false },
        { "--translate", OP_TRANSLATE, false }, { "--frame", OP_FRAME, true }, { "--code", OP_CODE, true }, { "--code-table", OP_CODE_TABLE, true },
        { "--repeats", OP_REPEATS, true }, { "--min-repeat", OP_MIN_REPEAT, true }, { "--whole-units", OP_WHOLE_UNITS, false },
        { "--trim", OP_TRIM, true }, { "--min-length", OP_MIN_LENGTH, true }, { "--max-ee", OP_MAX_EE, true }, { "--trim-table", OP_TRIM_TABLE, false },
        { "--adapter", OP_ADAPTER, true }, { "--adapter-errors", OP_ADAPTER_ERRORS, true }, { "--min-overlap", OP_MIN_OVERLAP, true }, { "--clip-table", OP_CLIP_TABLE, false },
        { "--dedup", OP_DEDUP, false }, { "--either-strand", OP_EITHER_STRAND, false }, { "--dedup-table", OP_DEDUP_TABLE, false },
        { "--screen", OP_SCREEN, true }, { "--screen-k", OP_SCREEN_K, true }, { "--min-hits", OP_MIN_HITS, true }, { "--keep-matched", OP_KEEP_MATCHED, false },
        { "--forward-only", OP_FORWARD_ONLY, false }, { "--screen-table", OP_SCREEN_TABLE, false } };
    for (int i = 1; i < argc; i++) {
        char *arg = argv[i];
        if (arg[0] != '-') {
            if (in_file_path) die("can process only one file at a time\n");
            if (!*arg) die("empty input path specified\n");
            in_file_path = arg; continue;
        }
        size_t k = 0;
        const size_t n_types = sizeof types / sizeof types[0], n_opts = sizeof option_table / sizeof option_table[0];
        while (k < n_types && strcmp(arg, types[k].name)) k++;
        if (k < n_types) { set_out_type(types[k].t); continue; }
        k = 0;
        while (k < n_opts && !(!strcmp(arg, option_table[k].name) && (!option_table[k].value || i < argc - 1))) k++;
        if (k == n_opts) die("unknown or incomplete argument \"%s\"\n", arg);
        char *v = option_table[k].value ? argv[++i] : NULL;
        switch (option_table[k].op) {
        case OP_LINE_LENGTH: set_line_length(v); break;
        case OP_OUT: if (out_file_path) die("double --out parameter\n"); if (!*v) die("empty --out parameter\n"); out_file_path = v; break;
        case OP_NO_MASK: use_mask = false; break;
        case OP_IGNORED: break;
        case OP_HELP: show_help(); exit(0);
        case OP_VERBOSE: verbose = true; break;
        case OP_VERSION: print_version = true; break;
        case OP_STDOUT: force_stdout = true; break;
        case OP_REGION: add_region(v, false); break;
        case OP_RC_REGION: add_region(v, true); break;
        case OP_REVCOMP: revcomp = true; break;
        case OP_RECORDS: add_records(v); break;
        case OP_LOCATE: add_locate(v); break;
        case OP_STRAND: set_strand(v); break;
        case OP_MISMATCHES: set_mismatches(v); break;
        case OP_COMPOSITION: composition = true; break;
        case OP_WINDOW: comp_window = positive_number("--window", "bases", v); window_given = true; break;
        case OP_QUALITY: quality = true; break;
        case OP_CYCLES: qual_cycles = positive_number("--cycles", "read positions", v); cycles_given = true; break;
        case OP_RUNS: set_runs(v); break;
        case OP_MASKED_RUNS: masked_runs = true; break;
        case OP_MIN_RUN: min_run = positive_number("--min-run", "bases", v); min_run_given = true; break;
        case OP_EACH: runs_each = true; break;
        case OP_KMERS: set_kmers(v); break;
        case OP_CANONICAL: kmers_canonical = true; break;
        case OP_PER_RECORD: kmers_per_record = true; break;
        case OP_ORFS: orfs = true; break;
        case OP_MIN_ORF: min_orf = positive_number("--min-orf", "bases", v); min_orf_given = true; break;
        case OP_STOPS: set_codons("--stops", v, &orf_stops_text, &orf_stops); break;
        case OP_STARTS: set_codons("--starts", v, &orf_starts_text, &orf_starts); break;
        case OP_STOP_TO_STOP: stop_to_stop = true; break;
        case OP_CLOSED: orfs_closed = true; break;
        case OP_SPLIT_UNKNOWN: orfs_split = true; break;
        case OP_TRANSLATE: translate = true; break;
        case OP_FRAME: set_frames(v); break;
        case OP_CODE: set_code(v); break;
        case OP_CODE_TABLE: set_code_table(v); break;
        case OP_REPEATS: set_repeats(v); break;
        case OP_MIN_REPEAT: min_repeat = positive_number("--min-repeat", "bases", v); min_repeat_given = true; break;
        case OP_WHOLE_UNITS: whole_units = true; break;
        case OP_TRIM: set_trim(v); break;
        case OP_MIN_LENGTH: trim_opts.min_len = positive_number("--min-length", "bases", v); min_length_given = true; break;
        case OP_MAX_EE: set_max_ee(v); break;
        case OP_TRIM_TABLE: trim_table = true; break;
        case OP_ADAPTER: add_adapter(v); break;
        case OP_ADAPTER_ERRORS: set_adapter_errors(v); break;
        case OP_MIN_OVERLAP: set_min_overlap(v); break;
        case OP_CLIP_TABLE: clip_table = true; break;
        case OP_DEDUP: dedup = true; break;
        case OP_EITHER_STRAND: either_strand = true; break;
        case OP_DEDUP_TABLE: dedup_table = true; break;
        case OP_SCREEN: set_screen(v); break;
        case OP_SCREEN_K: set_screen_k(v); break;
        case OP_MIN_HITS: screen_opts.min_hits = positive_number("--min-hits", "k-mers", v); min_hits_given = true; break;
        case OP_KEEP_MATCHED: keep_matched = true; break;
        case OP_FORWARD_ONLY: forward_only = true; break;
        case OP_SCREEN_TABLE: screen_table = true; break;
        }
    }
    if (print_version) {
        msg("unnaf - NAF decompressor, version " VERSION ", " DATE "\nCopyright (c) " COPYRIGHT_YEARS " Kirill Kryukov\n");
        if (verbose) msg("MI355X path: libnaf_gpu (HIP, gfx950), zstd frames decoded on the GPU\n");
        exit(0);
    }
    if (force_stdout && out_file_path) die("-c and -o arguments can't be used together\n");
    /* row by row: a message's place among the others is part of what the program does */
    fill_modes();
    for (const table_mode *m = modes; m < modes + N_MODES; m++) {
        for (const satellite *s = m->sat; s->refusal; s++) if (s->given && !s->fits) die("%s", s->refusal);
        if (m->early) m->early();
        if (!m->asked) continue;
        if (m->type_first) refuse_output_type(m);
        for (const table_mode *e = modes; e < m; e++)
            if (e->asked && !(e == &modes[M_ORFS] && m == &modes[M_TRANSLATE]) && !(e == &modes[M_CLIP] && m == &modes[M_TRIM]) &&
                !(e == &modes[M_DEDUP] && (m == &modes[M_CLIP] || m == &modes[M_TRIM])) &&
                !(e == &modes[M_SCREEN] && (m == &modes[M_DEDUP] || m == &modes[M_CLIP] || m == &modes[M_TRIM]))) die("%s and %s can't be used together\n", m->name, e->name);
        refuse_output_type(m);
        if (m->own) m->own(m);
        if (m->one_selection) one_whole_selection(m);
    }
    if ((n_selections || revcomp) && !(out_type == UNDECIDED || out_type == FASTA || out_type == FASTQ || out_type == SEQ || out_type == SEQUENCES))
        die("--region can be used only with sequence output\n");
    if (revcomp && !n_selections) die("--revcomp can be used only with --region or --records\n");
    if (revcomp) for (size_t k = 0; k < n_selections; k++) selections[k].rc = true;        /* (an --rc-region stays reverse: no double flip) */
}

static const unsigned char *naf; static size_t naf_len; static naf_gpu_header H; static void *d_naf = NULL;

static int naf_fd = -1;            /* a regular file: mapped for the header walk and the title, read into HBM by the I/O lanes */
static void upload_to(naf_gpu_ctx *c, void **d)
{
    CTX_TRY(c, naf_gpu_malloc(c, naf_len + 64, d));
    if (naf_fd >= 0) CTX_TRY(c, naf_gpu_read_file(c, naf_fd, 0, naf_len, *d));
    else { CTX_TRY(c, naf_gpu_upload(c, *d, naf, naf_len)); CTX_TRY(c, naf_gpu_synchronize(c)); }
}
static void upload(void) { gpu_open(); if (d_naf) return; upload_to(gpu, &d_naf); phase("archive upload"); }

static unsigned char *load_section(int i, const char *what)
{
    upload();
    unsigned long long n = H.orig_size[i];
    void *d; GPU_TRY(naf_gpu_malloc(gpu, n + 64, &d));
    size_t got = 0;
    int rc = naf_gpu_zstd_decompress(gpu, (const char *)d_naf + H.payload_off[i], H.comp_size[i], 0, d, n, &got);
    if (rc || got != n) die("can't decompress %s\n", what);
    unsigned char *h = (unsigned char *)malloc(n + 1);
    if (!h) die("can't allocate %llu bytes\n", n + 1);
    GPU_TRY(naf_gpu_download(gpu, h, d, n)); h[n] = 0;
    naf_gpu_free(gpu, d);
    return h;
}

/* ids / names: N strings, each with its terminator inside the section (input.c:145-200: "not 0-terminated", then the walk that
 * stops at "can't read id %llu" when the section holds fewer than N of them -- "currupted" is the reference's spelling for ids) */
static unsigned char *load_strings(int i, const char *what, unsigned long long n_strings)
{
    unsigned long long n = H.orig_size[i];
    if (n == 0) die("corrupted %s - not 0-terminated\n", what);
    unsigned char *b = load_section(i, what);
    if (b[n - 1] != 0) die("corrupted %s - not 0-terminated\n", what);
    unsigned long long have = 0;
    for (const unsigned char *p = b, *e = b + n; p < e && have < n_strings; have++) p = (const unsigned char *)memchr(p, 0, (size_t)(e - p)) + 1;
    if (have < n_strings) { if (i == 0) die("currupted ids - can't read id %llu\n", have); else die("corrupted names - can't read name %llu\n", have); }
    return b;
}

/* ---- text output --------------------------------------------------------------------------------------------------------------
 * The text is produced in byte ranges (naf_gpu_unnaf_range): never more than RANGE bytes of it are resident, so archives whose
 * text exceeds HBM decode too, and with NAF_GPUS=a,b,... every device takes a contiguous share of the text and writes it into
 * its place of the output file on its own (per-GPU D2H + pwrite: when the consumer is the host there is nothing to gather over
 * xGMI first).  A pipe gets the ranges in order from one device. */
static size_t range_bytes(void)
{
    const char *e = getenv("NAF_GPU_RANGE_BYTES");
    unsigned long long v = e ? strtoull(e, NULL, 10) : 0;
    if (v < 4096) v = (unsigned long long)16 << 30;
    return (size_t)(v & ~4095ull);
}
typedef struct { int k, n, device; naf_gpu_unnaf_opts o; size_t total, lo, hi; off_t file_at; naf_gpu_ctx *c; } text_job;
static void *text_worker(void *arg)
{
    text_job *j = (text_job *)arg;
    naf_gpu_ctx *c = j->c;
    void *d_arc = d_naf;
    if (!c) {                                                   /* a device of its own: context and a copy of the archive */
        c = ctx_open(j->device);
        upload_to(c, &d_arc);
    }
    const size_t R = range_bytes(), span = j->hi - j->lo, cap = span < R ? span : R;
    void *d; CTX_TRY(c, naf_gpu_malloc(c, cap + 64, &d));
    for (size_t b = j->lo; b < j->hi; b += cap) {
        size_t e = b + cap < j->hi ? b + cap : j->hi, got = 0;
        if (j->n == 1 && cap == j->total) CTX_TRY(c, naf_gpu_unnaf(c, d_arc, naf_len, &j->o, d, cap, &got));       /* everything at once: the whole-text call overlaps its side streams */
        else CTX_TRY(c, naf_gpu_unnaf_range(c, d_arc, naf_len, &j->o, b, e, d, cap, &got));
        if (got != e - b) die("can't decompress sequence\n");
        if (j->n == 1 && getenv("NAF_GPU_CLI_TIMING")) { CTX_TRY(c, naf_gpu_synchronize(c)); phase("unnaf on the GPU (waited for: timing only)"); }
        CTX_TRY(c, naf_gpu_write_file(c, fileno(OUT), (uint64_t)j->file_at + b, d, got));
    }
    naf_gpu_free(c, d);
    if (c != gpu) { naf_gpu_free(c, d_arc); naf_gpu_shutdown(c); }
    return NULL;
}

static void run_text(int mode, int masking_allowed)
{
    upload();
    naf_gpu_unnaf_opts o = { mode, masking_allowed && use_mask, line_length_is_specified ? requested_line_length : -1 };
    size_t n = 0; GPU_TRY(naf_gpu_unnaf_size(gpu, d_naf, naf_len, &o, &n));
    if (!n) return;
    phase("size");
    fflush(OUT);
    off_t at = fd_pwrite_pos(fileno(OUT));                   /* -1: a pipe, or a file opened for appending (`>>`): ranges in order from one device */
    if (at >= 0) {
        devices_parse();
        int nd = n_devs; if ((size_t)nd > n / 4096 + 1) nd = (int)(n / 4096 + 1);
        size_t per = ((n + (size_t)nd - 1) / (size_t)nd + 4095) & ~(size_t)4095;
        text_job jobs[MAX_DEVS]; pthread_t th[MAX_DEVS];
        for (int k = 0; k < nd; k++) {
            size_t lo = (size_t)k * per < n ? (size_t)k * per : n, hi = lo + per < n ? lo + per : n;
            jobs[k] = (text_job){ k, nd, dev_ids[k], o, n, lo, hi, at, k == 0 ? gpu : NULL };
        }
        for (int k = 1; k < nd; k++) if (pthread_create(&th[k], NULL, text_worker, &jobs[k]) != 0) die("can't start a device thread\n");
        text_worker(&jobs[0]);
        for (int k = 1; k < nd; k++) pthread_join(th[k], NULL);
        if (lseek(fileno(OUT), at + (off_t)n, SEEK_SET) < 0) die("can't write to file - disk full?\n");
        phase("unnaf on the GPU + download + write");
        return;
    }
    const size_t R = range_bytes(), cap = n < R ? n : R;
    void *d; GPU_TRY(naf_gpu_malloc(gpu, cap + 64, &d));
    if (cap == n) {                                             /* the whole text at once: one pass over the side streams */
        size_t got = 0; GPU_TRY(naf_gpu_unnaf(gpu, d_naf, naf_len, &o, d, n, &got));
        GPU_TRY(naf_gpu_synchronize(gpu)); phase("unnaf on the GPU");
        write_from_device(OUT, d, got);
    } else for (size_t b = 0; b < n; b += cap) {
        size_t e = b + cap < n ? b + cap : n, got = 0;
        GPU_TRY(naf_gpu_unnaf_range(gpu, d_naf, naf_len, &o, b, e, d, cap, &got));
        write_from_device(OUT, d, got);
    }
    phase("download + write"); naf_gpu_free(gpu, d);
}

/* --records A-B against the archive's record count */
static void check_records(const selection *s)
{
    if (s->last > H.n_sequences) die("--records: sequence %llu requested, the archive has %llu\n", s->last, (unsigned long long)H.n_sequences);
}
/* where every table mode's runner starts: the archive on the device, and the one --records or --region that the mode allows as
 * records rng_first .. rng_first + rng_count; none = every record */
static uint64_t rng_first, rng_count;
static void table_range(bool has_ids)
{
    upload();
    rng_first = 0; rng_count = NAF_GPU_WHOLE;
    if (!n_selections) return;
    const selection *s = &selections[0];
    if (s->region) {
        uint64_t rec = UINT64_MAX;
        if (has_ids && H.n_sequences) GPU_TRY(naf_gpu_unnaf_find(gpu, d_naf, naf_len, s->region, strlen(s->region) + 1, 1, &rec));
        if (rec == UINT64_MAX) die("sequence \"%s\" not found\n", s->region);
        rng_first = rec; rng_count = 1;
    } else {
        check_records(s);
        rng_first = s->first - 1; rng_count = s->last - s->first + 1;
    }
}
/* the first column of their tables, per record: ids, or the stored names of an archive without ids (*text holds them; both are the caller's to free) */
static const char **record_names(bool has_ids, bool has_names, unsigned char **text)
{
    const unsigned long long N = H.n_sequences;
    *text = has_ids ? load_strings(0, "ids", N) : has_names ? load_strings(1, "names", N) : NULL;
    const char **name = (const char **)malloc((size_t)(N + 1) * sizeof *name); if (!name) die("can't allocate memory\n");
    const char *p = (const char *)*text;
    for (unsigned long long r = 0; r < N; r++) { name[r] = p ? p : ""; if (p) p += strlen(p) + 1; }
    return name;
}

/* --region / --records: ids to record numbers (naf_gpu_unnaf_find), then the segments' texts in command-line order
 * (naf_gpu_unnaf_select_stranded: --rc-region / --revcomp give a segment's reverse complement), on the first device.  Nothing is written before every id is found. */
static void *sel_buf = NULL; static size_t sel_cap = 0;
static void emit_segments(const naf_gpu_unnaf_opts *o, const naf_gpu_segment *segs, const uint8_t *strand, size_t n)
{
    /* a selection larger than the range buffer is produced in pieces of whole segments: halves until a piece fits (or is one segment) */
    /* (--translate: the same segments as protein, naf_gpu_unnaf_translate; --trim: as reads, naf_gpu_unnaf_select_reads) */
    size_t need = 0;
    if (translate) GPU_TRY(naf_gpu_unnaf_translate_size(gpu, d_naf, naf_len, o, &genetic_code, segs, strand, n, &need));
    else if (reads_selection) GPU_TRY(naf_gpu_unnaf_select_reads_size(gpu, d_naf, naf_len, o, segs, strand, n, &need));
    else GPU_TRY(naf_gpu_unnaf_select_stranded_size(gpu, d_naf, naf_len, o, segs, strand, n, &need));
    if (!need) return;
    if (need > range_bytes() && n > 1) { emit_segments(o, segs, strand, n / 2); emit_segments(o, segs + n / 2, strand ? strand + n / 2 : NULL, n - n / 2); return; }
    if (need > sel_cap) { if (sel_buf) naf_gpu_free(gpu, sel_buf); GPU_TRY(naf_gpu_malloc(gpu, need + 64, &sel_buf)); sel_cap = need; }
    size_t got = 0;
    if (translate) GPU_TRY(naf_gpu_unnaf_translate(gpu, d_naf, naf_len, o, &genetic_code, segs, strand, n, sel_buf, sel_cap, &got));
    else if (reads_selection) GPU_TRY(naf_gpu_unnaf_select_reads(gpu, d_naf, naf_len, o, segs, strand, n, sel_buf, sel_cap, &got));
    else GPU_TRY(naf_gpu_unnaf_select_stranded(gpu, d_naf, naf_len, o, segs, strand, n, sel_buf, sel_cap, &got));
    if (got != need) die("can't decompress sequence\n");
    write_from_device(OUT, sel_buf, got);
}
/* --translate: every segment of a selection becomes its frames, side by side in the order of --frame.  Frame f > 0 is the segment from its
 * base f - 1 on, frame -f its reverse complement from base f - 1 on (forward bases [begin, end - (f - 1)), strand 1); for a reverse selection
 * the two swap.  Frame 1 or -1 of a whole record stays the whole record (its stored header); a frame that has no base is left out. */
static void segments_to_frames(naf_gpu_segment **segs, uint8_t **strand, size_t *n_segs, bool *any_rc)
{
    const unsigned long long N = H.n_sequences;
    uint64_t *len = (uint64_t *)malloc((size_t)(N + 1) * sizeof *len), *off = (uint64_t *)malloc((size_t)(N + 2) * sizeof *off);
    naf_gpu_segment *out = (naf_gpu_segment *)malloc((*n_segs * n_frames + 1) * sizeof *out);
    uint8_t *ost = (uint8_t *)malloc(*n_segs * n_frames + 1);
    if (!len || !off || !out || !ost) die("can't allocate memory\n");
    naf_gpu_unnaf_opts o = { NAF_OUT_FASTA, 0, -1 };
    if (N) GPU_TRY(naf_gpu_unnaf_record_table(gpu, d_naf, naf_len, &o, 0, N, len, off));
    size_t m = 0;
    for (size_t k = 0; k < *n_segs; k++) {
        const naf_gpu_segment g = (*segs)[k];
        const bool whole = g.begin == 0 && g.end == NAF_GPU_WHOLE;
        const uint64_t L = g.record < N ? len[g.record] : 0, e = g.end < L ? g.end : L;
        for (size_t q = 0; q < n_frames; q++) {
            const uint64_t skip = (uint64_t)(frames[q] < 0 ? -frames[q] : frames[q]) - 1;
            const bool rc = (frames[q] < 0) != ((*strand)[k] != 0);
            if (skip == 0 && (whole || g.begin >= e)) { ost[m] = rc; out[m++] = g; }                  /* the segment as it is (one that selects nothing: the call says so) */
            else if (g.begin + skip < e) { ost[m] = rc; out[m++] = rc ? (naf_gpu_segment){ g.record, g.begin, e - skip } : (naf_gpu_segment){ g.record, g.begin + skip, e }; }
        }
    }
    *any_rc = false;
    for (size_t k = 0; k < m; k++) *any_rc = *any_rc || ost[k];
    free(len); free(off); free(*segs); free(*strand);
    *segs = out; *strand = ost; *n_segs = m;
}
static void run_select(int mode, bool has_ids)
{
    upload();
    const unsigned long long N = H.n_sequences;
    if (translate && !n_selections && N) add_selection(NULL, 1, N, false);        /* --translate without a selection: every record */
    /* the ids of the regions, looked up in one call */
    size_t n_regions = 0, ids_bytes = 0, n_segs = 0;
    for (size_t k = 0; k < n_selections; k++) {
        const selection *s = &selections[k];
        if (s->region) { size_t l; uint64_t b, e; naf_gpu_parse_region(s->region, &l, &b, &e); n_regions++; ids_bytes += l + 1; n_segs++; }
        else {
            check_records(s);
            n_segs += (size_t)(s->last - s->first + 1);
        }
    }
    char *ids = (char *)malloc(ids_bytes + 1); uint64_t *recs = (uint64_t *)malloc((n_regions + 1) * sizeof *recs);
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc((n_segs + 1) * sizeof *segs);
    uint8_t *strand = (uint8_t *)malloc(n_segs + 1); bool any_rc = false;
    if (!ids || !recs || !segs || !strand) die("can't allocate memory\n");
    size_t at = 0;
    for (size_t k = 0; k < n_selections; k++) if (selections[k].region) {
        size_t l; uint64_t b, e; naf_gpu_parse_region(selections[k].region, &l, &b, &e);
        memcpy(ids + at, selections[k].region, l); ids[at + l] = 0; at += l + 1;
    }
    if (n_regions) {
        if (!has_ids || N == 0) { size_t l; uint64_t b, e; const char *r = NULL; for (size_t k = 0; !r; k++) r = selections[k].region; naf_gpu_parse_region(r, &l, &b, &e); die("sequence \"%.*s\" not found\n", (int)l, r); }
        GPU_TRY(naf_gpu_unnaf_find(gpu, d_naf, naf_len, ids, ids_bytes, n_regions, recs));
    }
    size_t q = 0, m = 0;
    for (size_t k = 0; k < n_selections; k++) {
        const selection *s = &selections[k];
        if (s->region) {
            size_t l; uint64_t b, e; naf_gpu_parse_region(s->region, &l, &b, &e);
            if (recs[q] == UINT64_MAX) die("sequence \"%.*s\" not found\n", (int)l, s->region);
            strand[m] = s->rc; segs[m++] = (naf_gpu_segment){ recs[q++], b, e };
        } else for (unsigned long long r = s->first; r <= s->last; r++) { strand[m] = s->rc; segs[m++] = (naf_gpu_segment){ r - 1, 0, NAF_GPU_WHOLE }; }
        any_rc = any_rc || s->rc;
    }
    if (translate) segments_to_frames(&segs, &strand, &n_segs, &any_rc);
    naf_gpu_unnaf_opts o = { mode, mode != NAF_OUT_FASTQ && use_mask, line_length_is_specified ? requested_line_length : -1 };
    fflush(OUT);
    emit_segments(&o, segs, any_rc ? strand : NULL, n_segs);
    if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
    free(ids); free(recs); free(segs); free(strand);
}

/* ---- the table modes' runners ------------------------------------------------------------------------------------------------------
 * A table of rows is made on the device (a count call, then a fill call into a table of that size) and written as lines here, on the host,
 * from the downloaded rows, a chunk at a time -- text for people and scripts, not a hot path.  write_rows is what all of them share; a
 * runner is its count call, its fill call and its formatter of a chunk's lines. */
typedef struct {
    size_t row_bytes, chunk;                                /* of one row; rows per download */
    const char *what, *filled, *written;                    /* "can't decompress WHAT"; the phase() behind the fill call and behind the lines */
    uint64_t (*fill)(void *d_rows, size_t cap);             /* the library call that writes the table: the rows it wrote */
    void (*lines)(const void *rows, size_t m, uint64_t at, const char **name);      /* rows at .. at + m of the table, downloaded; name: per record, NULL if not wanted */
} row_table;
static void write_rows(const row_table *t, uint64_t n, bool names, bool has_ids, bool has_names)
{
    void *d_rows; GPU_TRY(naf_gpu_malloc(gpu, (size_t)n * t->row_bytes, &d_rows));
    if (t->fill(d_rows, (size_t)n) != n) die("can't decompress %s\n", t->what);
    phase(t->filled);
    unsigned char *text = NULL; const char **name = names ? record_names(has_ids, has_names, &text) : NULL;
    void *rows = malloc((n < t->chunk ? (size_t)n : t->chunk) * t->row_bytes); if (!rows) die("can't allocate memory\n");
    for (uint64_t a = 0; a < n; a += t->chunk) {
        const size_t m = n - a < t->chunk ? (size_t)(n - a) : t->chunk;
        GPU_TRY(naf_gpu_download(gpu, rows, (const char *)d_rows + a * t->row_bytes, m * t->row_bytes));
        t->lines(rows, m, a, name);
    }
    free(rows); free(name); free(text); naf_gpu_free(gpu, d_rows);
    phase(t->written);
}

/* --locate: BED6 lines of the hits (naf_gpu_unnaf_locate: two passes over the packed stream).  With --mismatches or a bracketed pattern the
 * near search (naf_gpu_unnaf_locate_near): a line carries the number of mismatches in column 5 and, as a 7th column, the pattern's letters
 * in upper case with the mismatched ones in lower case (from the hit's `where`). */
static struct { char *blob; size_t bytes, len[MAX_LOCATE]; char letters[MAX_LOCATE][33]; uint32_t budget[MAX_LOCATE]; } pat;      /* the patterns as the calls take them; their letters without brackets */
static uint64_t fill_hits(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_locate(gpu, d_naf, naf_len, pat.blob, pat.bytes, n_locate, locate_strands, rng_first, rng_count, (naf_gpu_hit *)d, cap, &got));
    return got;
}
static void hit_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    for (const naf_gpu_hit *x = (const naf_gpu_hit *)rows; x < (const naf_gpu_hit *)rows + m; x++) {
        if (x->record >= H.n_sequences || x->pattern >= n_locate) die("can't decompress sequence\n");
        fprintf(OUT, "%s\t%llu\t%llu\t%s\t0\t%c\n", name[x->record], (unsigned long long)x->begin, (unsigned long long)(x->begin + pat.len[x->pattern]),
                locate_patterns[x->pattern], x->strand ? '-' : '+');
    }
}
static uint64_t fill_near_hits(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_locate_near(gpu, d_naf, naf_len, pat.blob, pat.bytes, n_locate, pat.budget, locate_strands, rng_first, rng_count, (naf_gpu_near_hit *)d, cap, &got));
    return got;
}
static void near_hit_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    for (const naf_gpu_near_hit *x = (const naf_gpu_near_hit *)rows; x < (const naf_gpu_near_hit *)rows + m; x++) {
        if (x->record >= H.n_sequences || x->pattern >= n_locate) die("can't decompress sequence\n");
        const char *letters = pat.letters[x->pattern]; const size_t len = pat.len[x->pattern];
        char site[33];
        for (size_t j = 0; j < len; j++) { const char ch = letters[j]; const bool low = ch >= 'a' && ch <= 'z'; site[j] = (char)(x->where >> j & 1 ? (low ? ch : ch + 32) : (low ? ch - 32 : ch)); }
        site[len] = 0;
        fprintf(OUT, "%s\t%llu\t%llu\t%s\t%u\t%c\t%s\n", name[x->record], (unsigned long long)x->begin, (unsigned long long)(x->begin + len),
                letters, (unsigned)x->mismatches, x->strand ? '-' : '+', site);
    }
}
static void run_locate(bool has_ids, bool has_names)
{
    static const row_table exact = { sizeof(naf_gpu_hit), 1 << 20, "sequence", "locate: hits", "locate: download + BED lines", fill_hits, hit_lines },
                           near = { sizeof(naf_gpu_near_hit), 1 << 20, "sequence", "locate-near: hits", "locate-near: download + BED lines", fill_near_hits, near_hit_lines };
    const bool is_near = mismatches_given || locate_bracketed;
    table_range(has_ids);
    pat.bytes = 0; for (size_t k = 0; k < n_locate; k++) pat.bytes += strlen(locate_patterns[k]) + 1;
    pat.blob = (char *)malloc(pat.bytes + 1); if (!pat.blob) die("can't allocate memory\n");
    for (size_t k = 0, at = 0; k < n_locate; k++) {
        const size_t l = strlen(locate_patterns[k]);
        memcpy(pat.blob + at, locate_patterns[k], l + 1); at += l + 1;
        pat.len[k] = 0; for (const char *p = locate_patterns[k]; *p; p++) if (*p != '[' && *p != ']') pat.letters[k][pat.len[k]++] = *p;
        pat.letters[k][pat.len[k]] = 0; pat.budget[k] = locate_mismatches;
    }
    uint64_t n = 0;
    if (is_near) GPU_TRY(naf_gpu_unnaf_locate_near_count(gpu, d_naf, naf_len, pat.blob, pat.bytes, n_locate, pat.budget, locate_strands, rng_first, rng_count, &n, NULL));
    else GPU_TRY(naf_gpu_unnaf_locate_count(gpu, d_naf, naf_len, pat.blob, pat.bytes, n_locate, locate_strands, rng_first, rng_count, &n, NULL));
    phase(is_near ? "locate-near: count" : "locate: count");
    if (n) write_rows(is_near ? &near : &exact, n, true, has_ids, has_names);
    free(pat.blob);
}

/* --composition [--window N]: naf_gpu_unnaf_composition, one sweep over the packed stream */
static uint64_t fill_composition(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_composition(gpu, d_naf, naf_len, comp_window, use_mask ? NAF_GPU_COMP_MASK : 0, rng_first, rng_count, (naf_gpu_comp_row *)d, cap, &got, NULL));
    return got;
}
static void composition_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    for (const naf_gpu_comp_row *x = (const naf_gpu_comp_row *)rows; x < (const naf_gpu_comp_row *)rows + m; x++) {
        if (x->record >= H.n_sequences) die("can't decompress sequence\n");
        const unsigned long long A = x->n[8], Cc = x->n[4], G = x->n[2], T = x->n[1], Nn = x->n[15], gap = x->n[0];
        unsigned long long other = 0; for (int q = 0; q < 16; q++) other += x->n[q];
        other -= A + Cc + G + T + Nn + gap;
        fprintf(OUT, "%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t", name[x->record], (unsigned long long)x->begin, (unsigned long long)x->end,
                A, Cc, G, T, Nn, other, gap, (unsigned long long)x->masked, (unsigned long long)x->cpg);
        if (A + Cc + G + T) fprintf(OUT, "%.6f\n", (double)(Cc + G) / (double)(A + Cc + G + T)); else fprintf(OUT, "NA\n");
    }
}
static void run_composition(bool has_ids, bool has_names)
{
    static const row_table t = { sizeof(naf_gpu_comp_row), 1 << 18, "sequence", "composition: count", "composition: download + lines", fill_composition, composition_lines };
    table_range(has_ids);
    uint64_t n = 0;
    GPU_TRY(naf_gpu_unnaf_composition_rows(gpu, d_naf, naf_len, comp_window, rng_first, rng_count, &n));
    phase("composition: rows");
    fprintf(OUT, "#seq\tstart\tend\tA\tC\tG\t%c\tN\tother\tgap\tmasked\tCpG\tGC\n", H.seq_type == NAF_SEQ_RNA ? 'U' : 'T');
    if (n) write_rows(&t, n, true, has_ids, has_names);
}

/* --quality [--cycles N]: naf_gpu_unnaf_quality, one sweep over the quality stream; a row per read, or per bin of N read positions */
static uint64_t qual_far;                                           /* the longest selected read: one row per read position at the most */
static uint64_t fill_quality(void *d, size_t cap)
{
    uint64_t got_rec = 0, got_cyc = 0;
    if (cycles_given) GPU_TRY(naf_gpu_unnaf_quality(gpu, d_naf, naf_len, qual_cycles, rng_first, rng_count, NULL, 0, (naf_gpu_qual_row *)d, cap, &got_rec, &got_cyc, NULL, NULL));
    else GPU_TRY(naf_gpu_unnaf_quality(gpu, d_naf, naf_len, 0, rng_first, rng_count, (naf_gpu_qual_row *)d, cap, NULL, 0, &got_rec, &got_cyc, NULL, NULL));
    return cycles_given ? got_cyc : got_rec;
}
static void quality_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    const uint64_t W = qual_cycles, far = qual_far;
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_qual_row *x = (const naf_gpu_qual_row *)rows + k;
        if (cycles_given) {
            if (x->key != at + k) die("can't decompress quality\n");
            const unsigned long long b = x->key * W + 1, e = far - x->key * W > W ? (x->key + 1) * W : far;
            fprintf(OUT, "%llu\t%llu\t%llu\t", b, e, (unsigned long long)x->n);
        } else {
            if (x->key >= H.n_sequences) die("can't decompress quality\n");
            fprintf(OUT, "%s\t%llu\t", name[x->key], (unsigned long long)x->n);
        }
        if (x->n) fprintf(OUT, "%.4f\t%d\t%d", (double)x->sum / (double)x->n - 33.0, (int)x->min - 33, (int)x->max - 33); else fprintf(OUT, "NA\tNA\tNA");
        fprintf(OUT, "\t%llu\t%llu\t%.6f\n", (unsigned long long)x->n_q20, (unsigned long long)x->n_q30, (double)x->ee / 4294967296.0);
    }
}
static void run_quality(bool has_ids, bool has_names)
{
    static const row_table t = { sizeof(naf_gpu_qual_row), 1 << 18, "quality", "quality: count", "quality: download + lines", fill_quality, quality_lines };
    table_range(has_ids);
    uint64_t n_rec = 0;
    GPU_TRY(naf_gpu_unnaf_quality_rows(gpu, d_naf, naf_len, 1, rng_first, rng_count, &n_rec, &qual_far));
    const uint64_t n = cycles_given ? qual_far / qual_cycles + (qual_far % qual_cycles != 0) : n_rec;
    phase("quality: rows");
    fprintf(OUT, cycles_given ? "#cycle_begin\tcycle_end\tn\tmean\tmin\tmax\tq20\tq30\tee\n" : "#seq\tlength\tmean\tmin\tmax\tq20\tq30\tee\n");
    if (n) write_rows(&t, n, !cycles_given, has_ids, has_names);
}

/* --runs / --masked-runs: BED4 lines (naf_gpu_unnaf_runs: the packed stream's run starts and ends, paired by rank; the mask's toggle list) */
static int runs_flags(void) { return masked_runs ? NAF_GPU_RUNS_MASKED : runs_each ? NAF_GPU_RUNS_EACH : 0; }
static uint64_t fill_runs(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_runs(gpu, d_naf, naf_len, masked_runs ? 0 : runs_set, runs_flags(), min_run, rng_first, rng_count, (naf_gpu_run *)d, cap, &got, NULL));
    return got;
}
static void run_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    const char *letters = H.seq_type == NAF_SEQ_RNA ? "-UGKCYSBAWRDMHVN" : "-TGKCYSBAWRDMHVN";
    for (const naf_gpu_run *x = (const naf_gpu_run *)rows; x < (const naf_gpu_run *)rows + m; x++) {
        if (x->record >= H.n_sequences || x->code > 15) die("can't decompress sequence\n");
        fprintf(OUT, "%s\t%llu\t%llu\t", name[x->record], (unsigned long long)x->begin, (unsigned long long)x->end);
        if (masked_runs) fprintf(OUT, "mask\n"); else if (runs_each) fprintf(OUT, "%c\n", letters[x->code]); else fprintf(OUT, "%s\n", runs_class);
    }
}
static void run_runs(bool has_ids, bool has_names)
{
    static const row_table t = { sizeof(naf_gpu_run), 1 << 20, "sequence", "runs: rows", "runs: download + BED lines", fill_runs, run_lines };
    table_range(has_ids);
    uint64_t n = 0;
    GPU_TRY(naf_gpu_unnaf_runs_count(gpu, d_naf, naf_len, masked_runs ? 0 : runs_set, runs_flags(), min_run, rng_first, rng_count, &n, NULL));
    phase("runs: count");
    if (n) write_rows(&t, n, true, has_ids, has_names);
}

/* --repeats: naf_gpu_unnaf_repeats -- the run starts and ends of "equals the base p in front" per period, paired by rank and merged without a sort */
static uint64_t fill_repeats(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_repeats(gpu, d_naf, naf_len, &repeats_spec, whole_units ? NAF_GPU_REPEATS_WHOLE_UNITS : 0, min_repeat, rng_first, rng_count, (naf_gpu_repeat *)d, cap, &got, NULL, NULL));
    return got;
}
static void repeat_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    const char *letters = H.seq_type == NAF_SEQ_RNA ? "ACGU" : "ACGT";
    for (const naf_gpu_repeat *x = (const naf_gpu_repeat *)rows; x < (const naf_gpu_repeat *)rows + m; x++) {
        uint32_t cls;
        if (x->record >= H.n_sequences || x->end <= x->begin || naf_gpu_repeat_class(x->motif, x->period, &cls)) die("can't decompress sequence\n");
        char motif[17], cl[17];
        for (unsigned i = 0; i < x->period; i++) { motif[i] = letters[(x->motif >> (2 * i)) & 3]; cl[i] = letters[(cls >> (2 * i)) & 3]; }
        motif[x->period] = cl[x->period] = 0;
        fprintf(OUT, "%s\t%llu\t%llu\t%u\t%s\t%llu\t%s\n", name[x->record], (unsigned long long)x->begin, (unsigned long long)x->end, (unsigned)x->period, motif,
                (unsigned long long)((x->end - x->begin) / x->period), cl);
    }
}
static void run_repeats(bool has_ids, bool has_names)
{
    static const row_table t = { sizeof(naf_gpu_repeat), 1 << 20, "sequence", "repeats: rows", "repeats: download + lines", fill_repeats, repeat_lines };
    table_range(has_ids);
    uint64_t n = 0;
    GPU_TRY(naf_gpu_unnaf_repeats_count(gpu, d_naf, naf_len, &repeats_spec, whole_units ? NAF_GPU_REPEATS_WHOLE_UNITS : 0, min_repeat, rng_first, rng_count, &n, NULL, NULL));
    phase("repeats: count");
    if (n) write_rows(&t, n, true, has_ids, has_names);
}

/* --trim: naf_gpu_unnaf_trim -- one sweep over the quality stream, a row per read.  --trim-table writes the rows as lines; without it a
 * chunk's kept rows are the segments of a selection of reads (naf_gpu_unnaf_select_reads): the trimmed reads instead of the lines. */
static uint64_t *trim_len;                                          /* the lengths of records rng_first .. (--trim-table's second column) */
static uint64_t fill_trim(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_trim(gpu, d_naf, naf_len, &trim_opts, rng_first, rng_count, (naf_gpu_trim_row *)d, cap, &got, NULL));
    return got;
}
static void trim_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_trim_row *x = (const naf_gpu_trim_row *)rows + k;
        if (x->record != rng_first + at + k || x->end < x->begin || x->end > trim_len[at + k] || x->flags < 1 || x->flags > 6 || x->flags == 5) die("can't decompress quality\n");
        fprintf(OUT, "%s\t%llu\t%llu\t%llu\t%.6f\t%s\n", name[x->record], (unsigned long long)trim_len[at + k], (unsigned long long)x->begin, (unsigned long long)x->end,
                (double)x->ee / 4294967296.0, x->flags == NAF_GPU_TRIM_KEPT ? "kept" : x->flags == NAF_GPU_TRIM_SHORT ? "short" : x->flags == NAF_GPU_TRIM_ERRORS ? "errors" : "short,errors");
    }
}
/* the n kept stretches of a chunk as reads, in the output type asked for */
static void emit_reads(const naf_gpu_segment *segs, size_t n)
{
    const int mode = out_type == FASTA ? NAF_OUT_FASTA : out_type == FASTQ ? NAF_OUT_FASTQ : out_type == SEQ ? NAF_OUT_SEQ : NAF_OUT_SEQUENCES;
    naf_gpu_unnaf_opts o = { mode, mode != NAF_OUT_FASTQ && use_mask, line_length_is_specified ? requested_line_length : -1 };
    fflush(OUT);
    if (n) emit_segments(&o, segs, NULL, n);
}
static void trim_reads(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)name;
    const naf_gpu_trim_row *x = (const naf_gpu_trim_row *)rows;
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc((m + 1) * sizeof *segs); if (!segs) die("can't allocate memory\n");
    size_t n = 0;
    for (size_t k = 0; k < m; k++) {
        if (x[k].record != rng_first + at + k || x[k].end < x[k].begin) die("can't decompress quality\n");
        if (x[k].flags == NAF_GPU_TRIM_KEPT) segs[n++] = (naf_gpu_segment){ x[k].record, x[k].begin, x[k].end };
    }
    emit_reads(segs, n);
    free(segs);
}
static void run_trim(bool has_ids, bool has_names)
{
    static const row_table lines = { sizeof(naf_gpu_trim_row), 1 << 20, "quality", "trim: rows", "trim: download + lines", fill_trim, trim_lines },
                           reads = { sizeof(naf_gpu_trim_row), 1 << 20, "quality", "trim: rows", "trim: download + reads", fill_trim, trim_reads };
    if (!(H.flags & 1)) die("--trim reads the quality codes: the archive has no quality section\n");
    table_range(has_ids);
    const unsigned long long N = H.n_sequences;
    if (rng_first > N) die("can't decompress quality\n");
    const uint64_t n = rng_count == NAF_GPU_WHOLE ? N - rng_first : rng_count;
    if (trim_table) {
        fprintf(OUT, "#seq\tlength\tbegin\tend\tee\tstatus\n");
        if (!n) return;
        uint64_t *off = (uint64_t *)malloc((size_t)(n + 1) * sizeof *off); trim_len = (uint64_t *)malloc((size_t)n * sizeof *trim_len);
        if (!off || !trim_len) die("can't allocate memory\n");
        naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, 0, -1 };
        GPU_TRY(naf_gpu_unnaf_record_table(gpu, d_naf, naf_len, &o, rng_first, n, trim_len, off));
        free(off);
        write_rows(&lines, n, true, has_ids, has_names);
        free(trim_len); trim_len = NULL;
        return;
    }
    reads_selection = true;
    if (n) write_rows(&reads, n, false, has_ids, has_names);
    if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
}

/* --adapter: naf_gpu_unnaf_clip -- one sweep over the packed stream, a row per read.  With --trim the trim rows of the same reads are made
 * first (naf_gpu_unnaf_trim) and stay on the device: they are the clip call's bounds.  --clip-table writes the rows as lines; without it a
 * chunk's kept rows are the segments of a selection of reads, as for --trim. */
static struct { char *blob; size_t bytes; uint8_t budget[NAF_GPU_CLIP_MAX_ADAPTERS][33]; } clip;
static uint64_t fill_clip(void *d, size_t cap)
{
    uint64_t got = 0; void *d_bounds = NULL;
    if (trim_text) {
        GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_trim_row), &d_bounds));
        GPU_TRY(naf_gpu_unnaf_trim(gpu, d_naf, naf_len, &trim_opts, rng_first, rng_count, (naf_gpu_trim_row *)d_bounds, cap, &got, NULL));
        if (got != cap) die("can't decompress quality\n");
        phase("clip: trim rows");
    }
    GPU_TRY(naf_gpu_unnaf_clip(gpu, d_naf, naf_len, clip.blob, clip.bytes, n_adapters, &clip.budget[0][0], &clip_opts, rng_first, rng_count,
                               (const naf_gpu_trim_row *)d_bounds, (naf_gpu_clip_row *)d, cap, &got, NULL, NULL));
    if (d_bounds) naf_gpu_free(gpu, d_bounds);
    return got;
}
static void clip_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_clip_row *x = (const naf_gpu_clip_row *)rows + k;
        const uint32_t f = x->flags & 7u; const bool clipped = (x->flags & NAF_GPU_CLIP_CLIPPED) != 0;
        if (x->record != rng_first + at + k || x->end < x->begin || x->end > trim_len[at + k] || x->flags > 15 || f < 1 || f > 6 || f == 5 || clipped != (x->adapter < n_adapters)) die("can't decompress sequence\n");
        fprintf(OUT, "%s\t%llu\t%llu\t%llu\t", name[x->record], (unsigned long long)trim_len[at + k], (unsigned long long)x->begin, (unsigned long long)x->end);
        if (clipped) fprintf(OUT, "%u", (unsigned)x->adapter + 1); else fputc('.', OUT);
        fprintf(OUT, "\t%u\t%u\t%s\n", (unsigned)x->mismatches, (unsigned)x->overlap, f == NAF_GPU_TRIM_KEPT ? "kept" : f == NAF_GPU_TRIM_SHORT ? "short" : f == NAF_GPU_TRIM_ERRORS ? "errors" : "short,errors");
    }
}
static void clip_reads(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)name;
    const naf_gpu_clip_row *x = (const naf_gpu_clip_row *)rows;
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc((m + 1) * sizeof *segs); if (!segs) die("can't allocate memory\n");
    size_t n = 0;
    for (size_t k = 0; k < m; k++) {
        if (x[k].record != rng_first + at + k || x[k].end < x[k].begin) die("can't decompress sequence\n");
        if (x[k].flags & NAF_GPU_TRIM_KEPT) segs[n++] = (naf_gpu_segment){ x[k].record, x[k].begin, x[k].end };
    }
    emit_reads(segs, n);
    free(segs);
}
/* the adapters and their budgets as the clip call takes them (the caller frees clip.blob) */
static void clip_prepare(void)
{
    clip.bytes = 0; for (size_t k = 0; k < n_adapters; k++) clip.bytes += strlen(adapters[k]) + 1;
    clip.blob = (char *)malloc(clip.bytes + 1); if (!clip.blob) die("can't allocate memory\n");
    for (size_t k = 0, at = 0; k < n_adapters; k++) {
        const size_t l = strlen(adapters[k]);
        memcpy(clip.blob + at, adapters[k], l + 1); at += l + 1;
        if (naf_gpu_clip_budgets(adapter_num, adapter_den, (unsigned)l, clip.budget[k])) die("can't parse the value of --adapter parameter (1 to 32 IUPAC nucleotide letters)\n");
    }
    clip_opts.min_len = trim_opts.min_len;                           /* --min-length: one value for both steps */
}
static void run_clip(bool has_ids, bool has_names)
{
    static const row_table lines = { sizeof(naf_gpu_clip_row), 1 << 20, "sequence", "clip: rows", "clip: download + lines", fill_clip, clip_lines },
                           reads = { sizeof(naf_gpu_clip_row), 1 << 20, "sequence", "clip: rows", "clip: download + reads", fill_clip, clip_reads };
    if (trim_text && !(H.flags & 1)) die("--trim reads the quality codes: the archive has no quality section\n");
    if (out_type == FASTQ && !(H.flags & 1)) die("FASTQ output requested, but input has no qualities\n");
    table_range(has_ids);
    const unsigned long long N = H.n_sequences;
    if (rng_first > N) die("can't decompress sequence\n");
    const uint64_t n = rng_count == NAF_GPU_WHOLE ? N - rng_first : rng_count;
    clip_prepare();
    if (clip_table) {
        fprintf(OUT, "#seq\tlength\tbegin\tend\tadapter\tmismatches\toverlap\tstatus\n");
        if (n) {
            uint64_t *off = (uint64_t *)malloc((size_t)(n + 1) * sizeof *off); trim_len = (uint64_t *)malloc((size_t)n * sizeof *trim_len);
            if (!off || !trim_len) die("can't allocate memory\n");
            naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, 0, -1 };
            GPU_TRY(naf_gpu_unnaf_record_table(gpu, d_naf, naf_len, &o, rng_first, n, trim_len, off));
            free(off);
            write_rows(&lines, n, true, has_ids, has_names);
            free(trim_len); trim_len = NULL;
        }
    } else {
        reads_selection = true;
        if (n) write_rows(&reads, n, false, has_ids, has_names);
        if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
    }
    free(clip.blob);
}

/* --dedup: naf_gpu_unnaf_dedup -- the windows of all selected reads hashed in one sweep over the packed stream and compared, a row per read.
 * With --trim and / or --adapter the trim rows and then the clip rows of the same reads are made first and stay on the device: the last
 * of them are the dedup call's bounds, as in run_clip.  --dedup-table writes the rows as lines; without it a chunk's firsts are the
 * segments of a selection of reads, as for --trim. */
static uint64_t fill_dedup(void *d, size_t cap)
{
    uint64_t got = 0; void *d_trim = NULL, *d_clip = NULL;
    if (trim_text) {
        GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_trim_row), &d_trim));
        GPU_TRY(naf_gpu_unnaf_trim(gpu, d_naf, naf_len, &trim_opts, rng_first, rng_count, (naf_gpu_trim_row *)d_trim, cap, &got, NULL));
        if (got != cap) die("can't decompress quality\n");
        phase("dedup: trim rows");
    }
    if (n_adapters) {
        GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_clip_row), &d_clip));
        GPU_TRY(naf_gpu_unnaf_clip(gpu, d_naf, naf_len, clip.blob, clip.bytes, n_adapters, &clip.budget[0][0], &clip_opts, rng_first, rng_count,
                                   (const naf_gpu_trim_row *)d_trim, (naf_gpu_clip_row *)d_clip, cap, &got, NULL, NULL));
        if (got != cap) die("can't decompress sequence\n");
        phase("dedup: clip rows");
    }
    const naf_gpu_dedup_opts o = { either_strand ? NAF_GPU_DEDUP_BOTH_STRANDS : 0, d_clip ? NAF_GPU_DEDUP_BOUNDS_CLIP : NAF_GPU_DEDUP_BOUNDS_TRIM };
    GPU_TRY(naf_gpu_unnaf_dedup(gpu, d_naf, naf_len, &o, rng_first, rng_count, d_clip ? d_clip : d_trim, (naf_gpu_dedup_row *)d, cap, &got, NULL, NULL));
    if (d_trim) naf_gpu_free(gpu, d_trim);
    if (d_clip) naf_gpu_free(gpu, d_clip);
    return got;
}
static void dedup_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_dedup_row *x = (const naf_gpu_dedup_row *)rows + k;
        const uint32_t f = x->flags & 7u; const bool dup = (x->flags & NAF_GPU_DEDUP_DUPLICATE) != 0;
        if (x->record != rng_first + at + k || x->end < x->begin || x->end > trim_len[at + k] || x->first > x->record || x->first < rng_first || x->strand > 1 || x->flags > 31 ||
            (dup ? f != 0 : f < 1 || f > 6 || f == 5) || (x->copies == 0) != (!dup && f != NAF_GPU_TRIM_KEPT)) die("can't decompress sequence\n");
        fprintf(OUT, "%s\t%llu\t%llu\t%llu\t%s\t%llu\t%c\t%s\n", name[x->record], (unsigned long long)trim_len[at + k], (unsigned long long)x->begin, (unsigned long long)x->end,
                name[x->first], (unsigned long long)x->copies, x->strand ? '-' : '+',
                dup ? "duplicate" : f == NAF_GPU_TRIM_KEPT ? "first" : f == NAF_GPU_TRIM_SHORT ? "short" : f == NAF_GPU_TRIM_ERRORS ? "errors" : "short,errors");
    }
}
static void dedup_reads(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)name;
    const naf_gpu_dedup_row *x = (const naf_gpu_dedup_row *)rows;
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc((m + 1) * sizeof *segs); if (!segs) die("can't allocate memory\n");
    const bool bounds = trim_text || n_adapters;                    /* without them a first is its whole record, an empty one too */
    size_t n = 0;
    for (size_t k = 0; k < m; k++) {
        if (x[k].record != rng_first + at + k || x[k].end < x[k].begin) die("can't decompress sequence\n");
        if (x[k].flags & NAF_GPU_TRIM_KEPT) segs[n++] = bounds ? (naf_gpu_segment){ x[k].record, x[k].begin, x[k].end } : (naf_gpu_segment){ x[k].record, 0, NAF_GPU_WHOLE };
    }
    emit_reads(segs, n);
    free(segs);
}
static void run_dedup(bool has_ids, bool has_names)
{
    static const row_table lines = { sizeof(naf_gpu_dedup_row), 1 << 20, "sequence", "dedup: rows", "dedup: download + lines", fill_dedup, dedup_lines },
                           reads = { sizeof(naf_gpu_dedup_row), 1 << 20, "sequence", "dedup: rows", "dedup: download + reads", fill_dedup, dedup_reads };
    if (trim_text && !(H.flags & 1)) die("--trim reads the quality codes: the archive has no quality section\n");
    if (!dedup_table && out_type == FASTQ && !(H.flags & 1)) die("FASTQ output requested, but input has no qualities\n");
    table_range(has_ids);
    const unsigned long long N = H.n_sequences;
    if (rng_first > N) die("can't decompress sequence\n");
    const uint64_t n = rng_count == NAF_GPU_WHOLE ? N - rng_first : rng_count;
    if (n_adapters) clip_prepare();
    if (dedup_table) {
        fprintf(OUT, "#seq\tlength\tbegin\tend\tfirst\tcopies\tstrand\tstatus\n");
        if (n) {
            uint64_t *off = (uint64_t *)malloc((size_t)(n + 1) * sizeof *off); trim_len = (uint64_t *)malloc((size_t)n * sizeof *trim_len);
            if (!off || !trim_len) die("can't allocate memory\n");
            naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, 0, -1 };
            GPU_TRY(naf_gpu_unnaf_record_table(gpu, d_naf, naf_len, &o, rng_first, n, trim_len, off));
            free(off);
            write_rows(&lines, n, true, has_ids, has_names);
            free(trim_len); trim_len = NULL;
        }
    } else {
        reads_selection = true;
        if (n) write_rows(&reads, n, false, has_ids, has_names);
        if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
    }
    if (n_adapters) free(clip.blob);
}

/* --screen: naf_gpu_unnaf_screen -- the reference's k-mers in a table on the device, the windows of all selected reads probed in one sweep over
 * the packed stream, a row per read.  With --trim and / or --adapter the trim rows and then the clip rows are made first and are the screen
 * call's bounds; with --dedup the screen rows are the dedup call's, as trim rows, and the table written is dedup's.  Nothing but the last
 * table leaves the device -- and, for --screen-table with --dedup, the screen rows, whose hits the lines carry. */
static void *d_screen_ref = NULL; static size_t screen_ref_len = 0;
static naf_gpu_screen_row *screen_host = NULL;                      /* --screen-table with --dedup: the screen rows of records rng_first .. */
static uint64_t fill_screen(void *d, size_t cap)
{
    uint64_t got = 0; void *d_trim = NULL, *d_clip = NULL, *d_scr = d;
    if (trim_text) {
        GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_trim_row), &d_trim));
        GPU_TRY(naf_gpu_unnaf_trim(gpu, d_naf, naf_len, &trim_opts, rng_first, rng_count, (naf_gpu_trim_row *)d_trim, cap, &got, NULL));
        if (got != cap) die("can't decompress quality\n");
        phase("screen: trim rows");
    }
    if (n_adapters) {
        GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_clip_row), &d_clip));
        GPU_TRY(naf_gpu_unnaf_clip(gpu, d_naf, naf_len, clip.blob, clip.bytes, n_adapters, &clip.budget[0][0], &clip_opts, rng_first, rng_count,
                                   (const naf_gpu_trim_row *)d_trim, (naf_gpu_clip_row *)d_clip, cap, &got, NULL, NULL));
        if (got != cap) die("can't decompress sequence\n");
        phase("screen: clip rows");
    }
    if (dedup) GPU_TRY(naf_gpu_malloc(gpu, cap * sizeof(naf_gpu_screen_row), &d_scr));
    naf_gpu_screen_opts o = screen_opts;
    o.flags = (keep_matched ? NAF_GPU_SCREEN_KEEP_MATCHED : 0) | (forward_only ? NAF_GPU_SCREEN_FORWARD_ONLY : 0);
    o.bounds_kind = d_clip ? NAF_GPU_SCREEN_BOUNDS_CLIP : NAF_GPU_SCREEN_BOUNDS_TRIM;
    GPU_TRY(naf_gpu_unnaf_screen(gpu, d_naf, naf_len, d_screen_ref, screen_ref_len, &o, rng_first, rng_count, d_clip ? d_clip : d_trim, (naf_gpu_screen_row *)d_scr, cap, &got, NULL));
    if (d_trim) naf_gpu_free(gpu, d_trim);
    if (d_clip) naf_gpu_free(gpu, d_clip);
    if (dedup) {
        if (got != cap) die("can't decompress sequence\n");
        phase("screen: screen rows");
        if (screen_table) {
            screen_host = (naf_gpu_screen_row *)malloc((cap + 1) * sizeof *screen_host); if (!screen_host) die("can't allocate memory\n");
            GPU_TRY(naf_gpu_download(gpu, screen_host, d_scr, cap * sizeof *screen_host));
        }
        const naf_gpu_dedup_opts od = { either_strand ? NAF_GPU_DEDUP_BOTH_STRANDS : 0, NAF_GPU_DEDUP_BOUNDS_TRIM };
        GPU_TRY(naf_gpu_unnaf_dedup(gpu, d_naf, naf_len, &od, rng_first, rng_count, d_scr, (naf_gpu_dedup_row *)d, cap, &got, NULL, NULL));
        naf_gpu_free(gpu, d_scr);
    }
    return got;
}
static void screen_line(const char **name, uint64_t k, uint64_t record, uint64_t begin, uint64_t end, uint64_t hits, uint32_t flags, bool dup)
{
    const uint32_t f = flags & 6u;
    if (record != rng_first + k || end < begin || end > trim_len[k]) die("can't decompress sequence\n");
    fprintf(OUT, "%s\t%llu\t%llu\t%llu\t%llu\t%s\n", name[record], (unsigned long long)trim_len[k], (unsigned long long)begin, (unsigned long long)end, (unsigned long long)hits,
            f == NAF_GPU_TRIM_SHORT ? "short" : f == NAF_GPU_TRIM_ERRORS ? "errors" : f ? "short,errors" : dup ? "duplicate" : flags & NAF_GPU_SCREEN_MATCHED ? "matched" : "clean");
}
static void screen_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_screen_row *x = (const naf_gpu_screen_row *)rows + k;
        screen_line(name, at + k, x->record, x->begin, x->end, x->hits, x->flags, false);
    }
}
static void screen_dedup_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    for (size_t k = 0; k < m; k++) {
        const naf_gpu_dedup_row *x = (const naf_gpu_dedup_row *)rows + k; const naf_gpu_screen_row *s = screen_host + at + k;
        if (s->record != x->record || s->begin != x->begin || s->end != x->end) die("can't decompress sequence\n");
        screen_line(name, at + k, x->record, x->begin, x->end, s->hits, s->flags, (x->flags & NAF_GPU_DEDUP_DUPLICATE) != 0);
    }
}
static void screen_reads(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)name;
    const naf_gpu_screen_row *x = (const naf_gpu_screen_row *)rows;
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc((m + 1) * sizeof *segs); if (!segs) die("can't allocate memory\n");
    const bool bounds = trim_text || n_adapters;                    /* without them a kept read is its whole record, an empty one too */
    size_t n = 0;
    for (size_t k = 0; k < m; k++) {
        if (x[k].record != rng_first + at + k || x[k].end < x[k].begin) die("can't decompress sequence\n");
        if (x[k].flags & NAF_GPU_TRIM_KEPT) segs[n++] = bounds ? (naf_gpu_segment){ x[k].record, x[k].begin, x[k].end } : (naf_gpu_segment){ x[k].record, 0, NAF_GPU_WHOLE };
    }
    emit_reads(segs, n);
    free(segs);
}
static void run_screen(bool has_ids, bool has_names)
{
    static const row_table lines = { sizeof(naf_gpu_screen_row), 1 << 20, "sequence", "screen: rows", "screen: download + lines", fill_screen, screen_lines },
                           dlines = { sizeof(naf_gpu_dedup_row), 1 << 20, "sequence", "screen: rows", "screen: download + lines", fill_screen, screen_dedup_lines },
                           reads = { sizeof(naf_gpu_screen_row), 1 << 20, "sequence", "screen: rows", "screen: download + reads", fill_screen, screen_reads },
                           dreads = { sizeof(naf_gpu_dedup_row), 1 << 20, "sequence", "screen: rows", "screen: download + reads", fill_screen, dedup_reads };     /* (the firsts among the kept reads: dedup's rows) */
    if (trim_text && !(H.flags & 1)) die("--trim reads the quality codes: the archive has no quality section\n");
    if (!screen_table && out_type == FASTQ && !(H.flags & 1)) die("FASTQ output requested, but input has no qualities\n");
    FILE *R = fopen(screen_ref, "rb");
    if (!R) die("can't open the --screen reference file\n");
    unsigned char *ref = read_all(R, &screen_ref_len); fclose(R);
    naf_gpu_header RH; char eb[128] = "";
    if (naf_gpu_parse_header_host(ref, screen_ref_len, &RH, eb)) die("--screen reference: %s", eb);
    if (RH.seq_type >= NAF_SEQ_PROTEIN) die("reads cannot be screened in %s sequences\n", RH.seq_type == NAF_SEQ_PROTEIN ? "protein" : "text");
    table_range(has_ids);
    const unsigned long long N = H.n_sequences;
    if (rng_first > N) die("can't decompress sequence\n");
    const uint64_t n = rng_count == NAF_GPU_WHOLE ? N - rng_first : rng_count;
    GPU_TRY(naf_gpu_malloc(gpu, screen_ref_len + 64, &d_screen_ref));
    GPU_TRY(naf_gpu_upload(gpu, d_screen_ref, ref, screen_ref_len)); GPU_TRY(naf_gpu_synchronize(gpu));
    free(ref);
    phase("screen: reference upload");
    if (n_adapters) clip_prepare();
    if (screen_table) {
        fprintf(OUT, "#seq\tlength\tbegin\tend\thits\tstatus\n");
        if (n) {
            uint64_t *off = (uint64_t *)malloc((size_t)(n + 1) * sizeof *off); trim_len = (uint64_t *)malloc((size_t)n * sizeof *trim_len);
            if (!off || !trim_len) die("can't allocate memory\n");
            naf_gpu_unnaf_opts o = { NAF_OUT_SEQUENCES, 0, -1 };
            GPU_TRY(naf_gpu_unnaf_record_table(gpu, d_naf, naf_len, &o, rng_first, n, trim_len, off));
            free(off);
            write_rows(dedup ? &dlines : &lines, n, true, has_ids, has_names);
            free(trim_len); trim_len = NULL; free(screen_host); screen_host = NULL;
        }
    } else {
        reads_selection = true;
        if (n) write_rows(dedup ? &dreads : &reads, n, false, has_ids, has_names);
        if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
    }
    if (n_adapters) free(clip.blob);
    naf_gpu_free(gpu, d_screen_ref); d_screen_ref = NULL;
}

/* --orfs: naf_gpu_unnaf_orfs -- the stops, starts and record bounds of the packed stream as six lists, a stretch between two neighbours of one
 * list.  With --translate a chunk's rows are the segments: their proteins instead of the lines. */
static int orfs_flags(void) { return (orfs_split ? NAF_GPU_ORF_SPLIT_UNKNOWN : 0) | (orfs_closed ? NAF_GPU_ORF_CLOSED : 0); }
static uint64_t fill_orfs(void *d, size_t cap)
{
    uint64_t got = 0;
    GPU_TRY(naf_gpu_unnaf_orfs(gpu, d_naf, naf_len, orf_stops, orf_starts, min_orf, locate_strands, orfs_flags(), rng_first, rng_count, (naf_gpu_orf *)d, cap, &got, NULL));
    return got;
}
static void orf_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at;
    for (const naf_gpu_orf *x = (const naf_gpu_orf *)rows; x < (const naf_gpu_orf *)rows + m; x++) {
        if (x->record >= H.n_sequences || x->strand > 1 || x->frame > 2 || x->end <= x->begin) die("can't decompress sequence\n");
        fprintf(OUT, "%s\t%llu\t%llu\t%c%u\t%llu\t%c\t%s\n", name[x->record], (unsigned long long)x->begin, (unsigned long long)x->end, x->strand ? '-' : '+', x->frame + 1u,
                (unsigned long long)((x->end - x->begin) / 3), x->strand ? '-' : '+', (x->flags & NAF_GPU_ORF_STOP3) ? "stop" : "open");
    }
}
static void orf_proteins(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)at; (void)name;
    const naf_gpu_orf *x = (const naf_gpu_orf *)rows;
    naf_gpu_segment *segs = (naf_gpu_segment *)malloc(m * sizeof *segs); uint8_t *strand = (uint8_t *)malloc(m);
    if (!segs || !strand) die("can't allocate memory\n");
    for (size_t k = 0; k < m; k++) {
        if (x[k].record >= H.n_sequences || x[k].strand > 1 || x[k].end <= x[k].begin) die("can't decompress sequence\n");
        segs[k] = (naf_gpu_segment){ x[k].record, x[k].begin, x[k].end }; strand[k] = (uint8_t)x[k].strand;
    }
    naf_gpu_unnaf_opts o = { NAF_OUT_FASTA, 0, line_length_is_specified ? requested_line_length : -1 };
    fflush(OUT);
    emit_segments(&o, segs, strand, m);
    free(segs); free(strand);
}
static void run_orfs(bool has_ids, bool has_names)
{
    static const row_table lines = { sizeof(naf_gpu_orf), 1 << 20, "sequence", "orfs: rows", "orfs: download + lines", fill_orfs, orf_lines },
                           proteins = { sizeof(naf_gpu_orf), 1 << 20, "sequence", "orfs: rows", "orfs: download + lines", fill_orfs, orf_proteins };
    table_range(has_ids);
    uint64_t n = 0;
    GPU_TRY(naf_gpu_unnaf_orfs_count(gpu, d_naf, naf_len, orf_stops, orf_starts, min_orf, locate_strands, orfs_flags(), rng_first, rng_count, &n, NULL, NULL));
    phase("orfs: count");
    if (n) write_rows(translate ? &proteins : &lines, n, true, has_ids, has_names);
    if (sel_buf) { naf_gpu_free(gpu, sel_buf); sel_buf = NULL; sel_cap = 0; }
}

/* --translate without --orfs: the selection's frames, through run_select */
static void run_translate(bool has_ids, bool has_names)
{
    (void)has_names;
    if (!((H.flags >> 1) & 1)) die("the archive stores no sequence to translate\n");
    run_select(NAF_OUT_FASTA, has_ids);
}

/* --kmers: the tables are made on the device (naf_gpu_unnaf_kmers: one sweep over the packed stream); the lines are formatted here, on the
 * host, from the downloaded counters, a chunk at a time -- the one table of a selection 2^20 counters at a time, the tables of --per-record
 * in calls of as many records as give 2^22 counters. */
static int kmers_flags(void) { return (kmers_canonical ? NAF_GPU_KMER_CANONICAL : 0) | (kmers_per_record ? NAF_GPU_KMER_PER_RECORD : 0); }
static void kmer_letters(uint64_t index, char *km)
{
    naf_gpu_kmer_text(kmers_k, index, km);
    if (H.seq_type == NAF_SEQ_RNA) for (char *q = km; *q; q++) if (*q == 'T') *q = 'U';
}
static uint64_t fill_kmers(void *d, size_t cap)                     /* the one table of a selection: its 4^K counters are the rows */
{
    uint64_t n_rows = 0, n_counters = 0;
    GPU_TRY(naf_gpu_unnaf_kmers(gpu, d_naf, naf_len, kmers_k, kmers_flags(), rng_first, rng_count, (uint64_t *)d, cap, NULL, 0, &n_rows, &n_counters, NULL));
    return n_rows == 1 && n_counters == 1ull << (2 * kmers_k) ? n_counters : UINT64_MAX;
}
static void kmer_lines(const void *rows, size_t m, uint64_t at, const char **name)
{
    (void)name;
    const uint64_t *cnt = (const uint64_t *)rows; char km[13];
    for (size_t k = 0; k < m; k++) if (cnt[k]) { kmer_letters(at + k, km); fprintf(OUT, "%s\t%llu\n", km, (unsigned long long)cnt[k]); }
}
static void run_kmers(bool has_ids, bool has_names)
{
    static const row_table one = { sizeof(uint64_t), 1 << 20, "sequence", "kmers: count", "kmers: download + lines", fill_kmers, kmer_lines };
    table_range(has_ids);
    const unsigned long long N = H.n_sequences;
    const unsigned K = kmers_k;
    const uint64_t nk = 1ull << (2 * K), first = rng_first;
    const int flags = kmers_flags();
    uint64_t n_rows = 0, n_counters = 0;
    GPU_TRY(naf_gpu_unnaf_kmers_rows(gpu, d_naf, naf_len, K, flags, rng_first, rng_count, &n_rows, &n_counters));
    phase("kmers: rows");
    if (!kmers_per_record) { if (n_rows) write_rows(&one, n_counters, false, has_ids, has_names); return; }
    char km[13];
    /* the columns: every k-mer, or the canonical ones */
    uint32_t *col = (uint32_t *)malloc((size_t)nk * sizeof *col); size_t n_col = 0; if (!col) die("can't allocate memory\n");
    fprintf(OUT, "#seq\tlength\tcounted");
    for (uint64_t x = 0; x < nk; x++) {
        unsigned k2; uint64_t can = x;
        kmer_letters(x, km);
        if (kmers_canonical) naf_gpu_kmer_index(km, 1, &k2, &can);
        if (can != x) continue;
        col[n_col++] = (uint32_t)x;
        fprintf(OUT, "\t%s", km);
    }
    fputc('\n', OUT);
    if (n_rows) {
        unsigned char *text; const char **name = record_names(has_ids, has_names, &text);
        const uint64_t total = n_rows, per_call = ((1ull << 22) >> (2 * K)) < total ? ((1ull << 22) >> (2 * K)) : total;
        void *d_counts, *d_rows;
        GPU_TRY(naf_gpu_malloc(gpu, (size_t)(per_call * nk) * 8, &d_counts)); GPU_TRY(naf_gpu_malloc(gpu, (size_t)per_call * sizeof(naf_gpu_kmer_row), &d_rows));
        uint64_t *cnt = (uint64_t *)malloc((size_t)(per_call * nk) * sizeof *cnt); naf_gpu_kmer_row *rows = (naf_gpu_kmer_row *)malloc((size_t)per_call * sizeof *rows);
        if (!cnt || !rows) die("can't allocate memory\n");
        for (uint64_t a = 0; a < total; a += per_call) {
            const uint64_t m = total - a < per_call ? total - a : per_call;
            uint64_t got_rows = 0, got_counters = 0;
            GPU_TRY(naf_gpu_unnaf_kmers(gpu, d_naf, naf_len, K, flags, first + a, m, (uint64_t *)d_counts, (size_t)(per_call * nk), (naf_gpu_kmer_row *)d_rows, (size_t)per_call,
                                        &got_rows, &got_counters, NULL));
            if (got_rows != m || got_counters != m * nk) die("can't decompress sequence\n");
            GPU_TRY(naf_gpu_download(gpu, cnt, d_counts, (size_t)(m * nk) * sizeof *cnt));
            GPU_TRY(naf_gpu_download(gpu, rows, d_rows, (size_t)m * sizeof *rows));
            for (uint64_t k = 0; k < m; k++) {
                const naf_gpu_kmer_row *x = &rows[k];
                if (x->record >= N) die("can't decompress sequence\n");
                fprintf(OUT, "%s\t%llu\t%llu", name[x->record], (unsigned long long)x->end, (unsigned long long)x->counted);
                for (size_t q = 0; q < n_col; q++) fprintf(OUT, "\t%llu", (unsigned long long)cnt[k * nk + col[q]]);
                fputc('\n', OUT);
            }
        }
        free(cnt); free(rows); free(name); free(text); naf_gpu_free(gpu, d_counts); naf_gpu_free(gpu, d_rows);
        phase("kmers: count + download + lines");
    }
    free(col);
}

int main(int argc, char **argv)
{
    prog_name = "unnaf";
    on_exit(done, NULL);
    parse_command_line(argc, argv);
    if (in_file_path == NULL && isatty(fileno(stdin))) { err("no input specified, use \"unnaf -h\" for help\n"); exit(0); }
    FILE *IN = in_file_path ? fopen(in_file_path, "rb") : stdin;
    if (!IN) die("can't open input file\n");
    phase("start");
    /* every output but the few that the header alone answers needs the device: its start runs beside the reading of the archive */
    if (!(out_type == FORMAT_NAME || out_type == PART_LIST || out_type == PART_SIZES || out_type == NUMBER_OF_SEQUENCES || out_type == TITLE || out_type == TOTAL_LENGTH)) { detach_teardown(); gpu_open_early(); }
    struct stat ist;
    if (fd_is_regular(fileno(IN)) && fstat(fileno(IN), &ist) == 0 && ist.st_size > 0) {
        void *m = mmap(NULL, (size_t)ist.st_size, PROT_READ, MAP_PRIVATE, fileno(IN), 0);
        if (m != MAP_FAILED) { naf = (const unsigned char *)m; naf_len = (size_t)ist.st_size; naf_fd = fileno(IN); }
    }
    if (naf_fd < 0) { naf = read_all(IN, &naf_len); if (IN != stdin) fclose(IN); }
    phase("read archive");
    char eb[128] = "";
    if (naf_gpu_parse_header_host(naf, naf_len, &H, eb)) die("%s", eb);
    int has_title = (H.flags >> 6) & 1, has_ids = (H.flags >> 5) & 1, has_names = (H.flags >> 4) & 1, has_lengths = (H.flags >> 3) & 1,
        has_mask = (H.flags >> 2) & 1, has_data = (H.flags >> 1) & 1, has_quality = H.flags & 1;
    static const char *tn[4] = { "DNA", "RNA", "protein", "text" };
    if (out_type == UNDECIDED) out_type = has_quality ? FASTQ : FASTA;
    if ((out_type == DNA || out_type == MASKED_DNA || out_type == UNMASKED_DNA) && H.seq_type != NAF_SEQ_DNA) die("input has not DNA, but %s data\n", tn[H.seq_type]);
    if (out_type == FOUR_BIT && H.seq_type >= NAF_SEQ_PROTEIN) die("input has no 4-bit encoded data, but %s sequences\n", tn[H.seq_type]);

    bool to_orig = has_quality ? (out_type == FASTA) : (out_type == FASTQ);
    char *auto_path = NULL;
    if (to_orig && !force_stdout && in_file_path && !out_file_path && isatty(fileno(stdout))) {
        size_t len = strlen(in_file_path);
        if (len > 4 && !strcmp(in_file_path + len - 4, ".naf") && in_file_path[len - 5] != '/' && in_file_path[len - 5] != '\\') {
            auto_path = (char *)malloc(len - 3); memcpy(auto_path, in_file_path, len - 4); auto_path[len - 4] = 0; out_file_path = auto_path;
        }
    }
    if (out_file_path && !force_stdout) { OUT = fopen(out_file_path, "wb"); if (!OUT) die("can't create output file\n"); created_output_file = true; }
    else OUT = stdout;
    bool large = out_type == IDS || out_type == NAMES || out_type == LENGTHS || out_type == MASK || out_type == FOUR_BIT || out_type == DNA ||
                 out_type == MASKED_DNA || out_type == UNMASKED_DNA || out_type == SEQ || out_type == FASTA || out_type == MASKED_FASTA ||
                 out_type == UNMASKED_FASTA || out_type == FASTQ;
    const table_mode *mode = asked_mode();
    if (large && !mode && !force_stdout && isatty(fileno(OUT)))
        die("output file not specified - please either specify output file with '-o' or '>', or use '-c' option to force writing to console\n");

    unsigned long long N = H.n_sequences;
    if (mode) {
        if (mode->protein && H.seq_type >= NAF_SEQ_PROTEIN) die(mode->protein, tn[H.seq_type]);
        mode->run(has_ids, has_names);
    }
    else if (n_selections) {
        if (out_type == FASTQ && !has_quality) die("FASTQ output requested, but input has no qualities\n");
        for (size_t k = 0; k < n_selections; k++) if (selections[k].rc && H.seq_type >= NAF_SEQ_PROTEIN) die("%s sequences have no reverse complement\n", tn[H.seq_type]);
        run_select(out_type == FASTA ? NAF_OUT_FASTA : out_type == FASTQ ? NAF_OUT_FASTQ : out_type == SEQ ? NAF_OUT_SEQ : NAF_OUT_SEQUENCES, has_ids);
    }
    else if (out_type == FORMAT_NAME) fprintf(OUT, "%s sequences%s in NAF format version %d\n", tn[H.seq_type], has_quality ? " with qualities" : "", H.version);
    else if (out_type == PART_LIST) {
        int printed = 0; const char *nm[7] = { "Title", "IDs", "Names", "Lengths", "Mask", "Data", "Quality" };
        int has[7] = { has_title, has_ids, has_names, has_lengths, has_mask, has_data, has_quality };
        for (int i = 0; i < 7; i++) if (has[i]) { fprintf(OUT, "%s%s", printed ? ", " : "", nm[i]); printed++; }
        fprintf(OUT, "\n");
    }
    else if (out_type == NUMBER_OF_SEQUENCES) fprintf(OUT, "%llu\n", N);
    else if (out_type == PART_SIZES) {
        if (has_title) fprintf(OUT, "Title: %llu\n", (unsigned long long)H.title_len);
        const char *nm[6] = { "IDs", "Names", "Lengths", "Mask", "Data", "Quality" };
        for (int i = 0; i < 6; i++) if (H.flags & (0x20 >> i))
            fprintf(OUT, "%s: %llu / %llu (%.3f%%)\n", nm[i], (unsigned long long)H.comp_size[i], (unsigned long long)H.orig_size[i], (double)H.comp_size[i] / (double)H.orig_size[i] * 100);
    }
    else if (out_type == TITLE) { if (has_title) fwrite(naf + H.title_off, 1, H.title_len, OUT); fputc('\n', OUT); }
    else if (N != 0) {
        if (out_type == IDS) { if (has_ids) { unsigned char *b = load_strings(0, "ids", N); const char *p = (const char *)b; for (unsigned long long i = 0; i < N; i++) { fprintf(OUT, "%s\n", p); p += strlen(p) + 1; } free(b); } }
        else if (out_type == NAMES) {
            if (has_ids || has_names) {
                unsigned char *a = has_ids ? load_strings(0, "ids", N) : NULL, *b = has_names ? load_strings(1, "names", N) : NULL;
                const char *p = (const char *)a, *q = (const char *)b;
                for (unsigned long long i = 0; i < N; i++) {
                    if (p) { fputs(p, OUT); p += strlen(p) + 1; }
                    if (q) { if (!a) fputs(q, OUT); else if (q[0]) { fputc(H.separator, OUT); fputs(q, OUT); } q += strlen(q) + 1; }
                    fputc('\n', OUT);
                }
                free(a); free(b);
            }
        }
        else if (out_type == LENGTHS) {
            if (has_lengths) { unsigned char *b = load_section(2, "lengths"); const unsigned int *u = (const unsigned int *)b; unsigned long long n = H.orig_size[2] / 4;
                for (unsigned long long i = 0; i < n; i++) { unsigned long long len = 0; while (i < n && u[i] == 4294967295u) { len += 4294967295llu; i++; } if (i < n) len += u[i]; fprintf(OUT, "%llu\n", len); } free(b); }
        }
        else if (out_type == TOTAL_LENGTH) { if (has_lengths) fprintf(OUT, "%llu\n", (unsigned long long)H.orig_size[4]); }
        else if (out_type == MASK) {
            if (has_mask) { unsigned char *b = load_section(3, "mask"); unsigned long long n = H.orig_size[3];
                for (unsigned long long i = 0; i < n; i++) { unsigned long long len = 0; while (i < n && b[i] == 255u) { len += 255llu; i++; } if (i < n) len += b[i]; fprintf(OUT, "%llu\n", len); } free(b); }
        }
        else if (out_type == TOTAL_MASK_LENGTH) {
            if (has_mask) { unsigned char *b = load_section(3, "mask"); unsigned long long t = 0; for (unsigned long long i = 0; i < H.orig_size[3]; i++) t += b[i]; fprintf(OUT, "%llu\n", t); free(b); }
            else fprintf(OUT, "0\n");
        }
        else if (out_type == FOUR_BIT) run_text(NAF_OUT_4BIT, 1);
        else if (out_type == DNA || out_type == SEQ || out_type == MASKED_DNA) run_text(NAF_OUT_SEQ, 1);
        else if (out_type == UNMASKED_DNA) run_text(NAF_OUT_SEQ, 0);
        else if (out_type == CHARCOUNT) { if (has_data) {          /* histogram of the --seq text (output.c:515-605), a byte range at a time */
                upload();
                naf_gpu_unnaf_opts o = { NAF_OUT_SEQ, use_mask, -1 }; size_t n = 0; GPU_TRY(naf_gpu_unnaf_size(gpu, d_naf, naf_len, &o, &n));
                const size_t R = range_bytes(), cap = n < R ? n : R;
                unsigned long long counts[256]; memset(counts, 0, sizeof counts);
                void *d; GPU_TRY(naf_gpu_malloc(gpu, cap + 64, &d));
                for (size_t b = 0; b < n; b += cap) {
                    size_t e = b + cap < n ? b + cap : n, got = 0;
                    if (cap == n) GPU_TRY(naf_gpu_unnaf(gpu, d_naf, naf_len, &o, d, n, &got));
                    else GPU_TRY(naf_gpu_unnaf_range(gpu, d_naf, naf_len, &o, b, e, d, cap, &got));
                    uint64_t cnt64[256]; GPU_TRY(naf_gpu_histogram(gpu, d, got, cnt64));
                    for (unsigned i = 0; i < 256; i++) counts[i] += cnt64[i];
                }
                for (unsigned i = 0; i < 33; i++) if (counts[i]) fprintf(OUT, "\\x%02X\t%llu\n", i, counts[i]);
                for (unsigned i = 33; i < 127; i++) if (counts[i]) fprintf(OUT, "%c\t%llu\n", (unsigned char)i, counts[i]);
                for (unsigned i = 127; i < 256; i++) if (counts[i]) fprintf(OUT, "\\x%02X\t%llu\n", i, counts[i]);
                naf_gpu_free(gpu, d); } }
        else if (out_type == SEQUENCES) run_text(NAF_OUT_SEQUENCES, 1);
        else if (out_type == FASTA || out_type == MASKED_FASTA) run_text(NAF_OUT_FASTA, 1);
        else if (out_type == UNMASKED_FASTA) run_text(NAF_OUT_FASTA, 0);
        else if (out_type == FASTQ) { if (!has_quality) die("FASTQ output requested, but input has no qualities\n"); run_text(NAF_OUT_FASTQ, 0); }
        else die("unknown output requested\n");
    }
    if (OUT != stdout) { if (fclose(OUT) != 0) die("can't close file - disk full?\n"); } else fflush(stdout);
    success = true;
    /* everything is written and closed: the process ends here, without the device-side teardown (freeing gigabytes of device memory,
     * streams, the runtime's own exit handlers: 0.1 - 0.2 s that nobody waits for; NAF_GPU_SLOW_EXIT=1 runs it) */
    trace_out(); fflush(NULL); detach_done(0);
    { const char *se = getenv("NAF_GPU_SLOW_EXIT"); if (!(se && se[0] == '1')) _exit(0); }
    return 0;
}
