// translate.h -- segments and ORFs as protein, translated from the packed 4-bit stream (naf_gpu_genetic_code_by_id, naf_gpu_genetic_code_parse,
// naf_gpu_genetic_code_stops, naf_gpu_codon_lut, naf_gpu_unnaf_translate_size, naf_gpu_unnaf_translate).  Part of emit.hip (included by it, behind
// orfs.h): the front of the call -- validation, header lines, line geometry, the sort and merge of the base intervals, the range decodes and
// their binding -- is select_run of emit_select.h with three bases to the byte; this file holds the genetic codes, the codon table and the
// kernel that writes the letters.
//
// The contract (include/naf_gpu.h carries it too):
//   code       aa[i] = the letter of the codon of index i under naf_gpu_kmer_index at K = 3 (A = 0, C = 1, G = 2, T/U = 3, first base most
//              significant); '*' = stop.
//   table      4096 letters, index (c0 << 8) | (c1 << 4) | c2 of the stored codes of "-TGKCYSBAWRDMHVN" in reading order: the letter all
//              expansions of the three codes agree on, else 'X'; "---" is '-', any other codon with a gap 'X'.
//   text       per segment the header line of naf_gpu_unnaf_select_stranded in FASTA mode, then floor(n / 3) letters from the segment's first
//              base in reading direction, wrapped at the line length counted in letters.
//
// The kernel reads the stream as it lies.  Three stored codes are twelve consecutive bits, c0 in the lowest nibble, so a codon is a 12-bit
// field of the stream and the table the kernel indexes is the contract's with the nibbles of the index turned round (tab[0 .. 4096)).  A
// reverse codon over forward bases o, o + 1, o + 2 reads comp(o + 2) comp(o + 1) comp(o), and the complement of a code is the code with
// its four bits reversed: a second table (tab[4096 .. 8192)) takes the same 12-bit field, so the reverse strand costs no instruction per
// codon -- its sixteen fields are loaded from the far end of the piece and the sixteen letters turned round in registers, as the
// selection turns its bases.  Both tables are made on the host per call (8 KiB uploaded) and copied into LDS once per workgroup of four
// wavefronts; a wavefront composes 4 KiB of text in four rounds of 64 lanes x 16 bytes, and a lane's 16 letters are 48 bases = 24 bytes of
// stream (25 at the odd nibble phase), loaded as three 8-byte words and a byte.
#pragma once

#define TR_WAVES 4u                          // wavefronts of a workgroup: 4 KiB of text each, one copy of the tables for all

// The 16 letters of the 48 bases from base b0 of the stream at seq (only the first n1 are kept by the caller): bytes [b0 / 2, b0 / 2 +
// nb) are needed, nb = ceil((3 n1 + b0 mod 2) / 2) <= 25, and at most seven more are read -- the slack behind every decoded range.
__device__ __forceinline__ void translate16(const u8 *t, const u8 *seq, u64 b0, u32 n1, u64 &lo, u64 &hi)
{
    const u8 *a = seq + (b0 >> 1);
    const u32 ph = (u32)b0 & 1u, nb = (3 * n1 + ph + 1) >> 1;
    u64 w[3] = { ld64(a), nb > 8 ? ld64(a + 8) : 0, nb > 16 ? ld64(a + 16) : 0 };
    if (ph) {
        const u64 w3 = nb > 24 ? (u64)a[24] : 0;
        w[0] = (w[0] >> 4) | (w[1] << 60); w[1] = (w[1] >> 4) | (w[2] << 60); w[2] = (w[2] >> 4) | (w3 << 60);
    }
    lo = 0; hi = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int bit = 12 * k, wd = bit >> 6, sh = bit & 63;
        u64 f = w[wd] >> sh;
        if (sh > 52) f |= w[wd + 1] << (64 - sh);                                 // (k = 5 and k = 10: a field across two words)
        const u64 letter = t[(u32)f & 0xFFFu];
        if (k < 8) lo |= letter << (8 * k); else hi |= letter << (8 * (k - 8));
    }
}

// One 16-byte chunk of the translation's text, piece by piece as select_chunk composes one of the selection's: a piece is n_main bytes of
// header or letters followed by at most one newline.  Letter j of a forward segment is the codon at bases g0 + 3 j ..; letter j of a reverse
// one the codon that ends at base g0 + n - 3 j, so a piece of n1 letters from letter j takes the 3 n1 bases that start at g0 + n - 3 (j + n1)
// -- never in front of the segment -- through the second table, and its letters are turned round.
template <bool RC>
__device__ __forceinline__ void translate_chunk(const EmitP &P, const u8 *tab, const SelSeg *sg, const u64 *seg_out, const u8 *hdr_text, u64 p0, u32 nbytes, u64 s, u32 Lp1_32, u8 *o)
{
    u64 so = seg_out[s], sn = seg_out[s + 1];
    SelSeg g = sg[s];
    u64 lo = 0, hi = 0; u32 pos = 0;
    while (pos < nbytes) {
        const u64 p = p0 + pos;
        while (p >= sn) { s++; so = sn; sn = seg_out[s + 1]; g = sg[s]; }            // (p < seg_out[S]: the loop ends inside the table)
        const u64 off = p - so, len = g.n / 3;                                     // len: the letters
        const u8 *src = nullptr; u64 j = 0; bool is_letters = false;
        u64 n_main = 0; u32 n_tc = 0;
        if (off < g.hl) { src = hdr_text + g.ho + off; n_main = g.hl - off; }
        else {
            const u64 q = off - g.hl;
            n_tc = 1;
            if (P.L == 0) { if (q < len) { is_letters = true; j = q; n_main = len - q; } }
            else {
                u64 line, col;
                if (Lp1_32 && (q >> 32) == 0) { const u32 l32 = (u32)q / Lp1_32; line = l32; col = (u32)q - l32 * Lp1_32; }
                else { line = q / (P.L + 1); col = q - line * (P.L + 1); }
                j = line * P.L + col;
                if (col != P.L && j < len) { is_letters = true; n_main = len - j < P.L - col ? len - j : P.L - col; }
            }
        }
        u32 rem = nbytes - pos;
        const u32 n1 = n_main < rem ? (u32)n_main : rem;
        if (n1) {
            u64 slo, shi;
            if (is_letters) {
                if (RC && (g.sub & SEL_RC)) { translate16(tab + 4096, g.seq, g.g0 + g.n - 3 * (j + n1), n1, slo, shi); reverse16(slo, shi, n1); }
                else translate16(tab, g.seq, g.g0 + 3 * j, n1, slo, shi);
            }
            else { slo = ld64(src); shi = n1 > 8 ? ld64(src + 8) : 0; }
            place16(lo, hi, slo, shi, pos, n1);
            pos += n1; rem -= n1;
        }
        if (n1 == n_main && rem && n_tc) { place16(lo, hi, '\n', 0, pos, 1); pos++; }
    }
    store_upto16(o, lo, hi, nbytes);
}

// A workgroup of TR_WAVES wavefronts: the tables into LDS (d_tab: 16-byte aligned, 4096 bytes, 8192 with RC), then one wavefront per 4 KiB
// tile of the text as in k_emit_select.  RC = true is the instantiation of a call with reverse segments.
template <bool RC>
__global__ __launch_bounds__(64 * TR_WAVES) void k_emit_translate(EmitP P, const u8 *d_tab, const SelSeg *sg, const u64 *seg_out, u64 S, const u8 *hdr_text, u64 total, u8 *out)
{
    __shared__ __attribute__((aligned(16))) u8 tab[RC ? 8192 : 4096];
    for (u32 i = threadIdx.x; i < sizeof tab / 16; i += 64 * TR_WAVES) ((uint4 *)tab)[i] = ((const uint4 *)d_tab)[i];
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    const u64 t0 = ((u64)xcd_block() * TR_WAVES + (threadIdx.x >> 6)) * 4096, t1 = t0 + 4096 < total ? t0 + 4096 : total;
    if (t0 >= total) return;
    const u64 s_lo = upper_bound_u64(seg_out, 0, S + 1, t0) - 1, s_hi = upper_bound_u64(seg_out, s_lo, S + 1, t1 - 1) - 1;
    const u32 Lp1_32 = (P.L + 1) >> 32 ? 0 : (u32)(P.L + 1);
#pragma unroll 1
    for (u32 k = 0; k < 4; k++) {
        const u64 p0 = t0 + k * 1024 + lane * 16;
        if (p0 >= t1) break;
        const u32 nbytes = t1 - p0 < 16 ? (u32)(t1 - p0) : 16u;
        const u64 s = s_lo == s_hi ? s_lo : upper_bound_u64(seg_out, s_lo, s_hi + 1, p0) - 1;
        translate_chunk<RC>(P, tab, sg, seg_out, hdr_text, p0, nbytes, s, Lp1_32, out + p0);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// Code 1 in the index order of naf_gpu_kmer_index (AAA AAC AAG AAT ACA ...), and the other built-in codes as their differences from it
static const char TR_STANDARD[65] = "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF";
static const struct { int id; const char *diff; } TR_CODES[] = {
    { 1, "" }, { 2, "AGA* AGG* ATAM TGAW" }, { 3, "ATAM CTTT CTCT CTAT CTGT TGAW" }, { 4, "TGAW" }, { 5, "AGAS AGGS ATAM TGAW" },
    { 6, "TAAQ TAGQ" }, { 9, "AAAN AGAS AGGS TGAW" }, { 10, "TGAC" }, { 11, "" }, { 12, "CTGS" }, { 13, "AGAG AGGG ATAM TGAW" },
    { 14, "AAAN AGAS AGGS TAAY TGAW" }, { 15, "TAGQ" }, { 16, "TAGL" }, { 21, "AAAN AGAS AGGS ATAM TGAW" }, { 22, "TCA* TAGL" },
    { 23, "TTA*" }, { 24, "AGAS AGGK TGAW" }, { 25, "TGAG" }, { 26, "CTGA" },
};

extern "C" int naf_gpu_genetic_code_by_id(int ncbi_id, naf_gpu_genetic_code *code)
{
    if (!code) return NAF_GPU_EARG;
    for (const auto &t : TR_CODES) {
        if (t.id != ncbi_id) continue;
        memcpy(code->aa, TR_STANDARD, 64);
        for (const char *p = t.diff; *p; p += p[4] ? 5 : 4) {                     // "XYZa": codon XYZ is letter a
            static const char acgt[] = "ACGT";
            const int i = 16 * (int)(strchr(acgt, p[0]) - acgt) + 4 * (int)(strchr(acgt, p[1]) - acgt) + (int)(strchr(acgt, p[2]) - acgt);
            code->aa[i] = p[3];
        }
        return 0;
    }
    return NAF_GPU_EARG;
}

extern "C" int naf_gpu_genetic_code_parse(const char *letters64, naf_gpu_genetic_code *code)
{
    if (!letters64 || !code || strlen(letters64) != 64) return NAF_GPU_EARG;
    char aa[64];
    for (int i = 0; i < 64; i++) {
        char ch = letters64[i];
        if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
        if (!((ch >= 'A' && ch <= 'Z') || ch == '*')) return NAF_GPU_EARG;
        aa[i] = ch;
    }
    memcpy(code->aa, aa, 64);
    return 0;
}

// the letters of a code are what the two calls above can have written: anything else is no code
static bool tr_code_ok(const naf_gpu_genetic_code *code)
{
    if (!code) return false;
    for (int i = 0; i < 64; i++) if (!((code->aa[i] >= 'A' && code->aa[i] <= 'Z') || code->aa[i] == '*')) return false;
    return true;
}

extern "C" int naf_gpu_genetic_code_stops(const naf_gpu_genetic_code *code, uint64_t *stops)
{
    if (!stops || !tr_code_ok(code)) return NAF_GPU_EARG;
    u64 s = 0;
    for (int i = 0; i < 64; i++) if (code->aa[i] == '*') s |= 1ull << i;
    *stops = s;
    return 0;
}

extern "C" int naf_gpu_codon_lut(const naf_gpu_genetic_code *code, uint8_t lut[4096])
{
    if (!lut || !tr_code_ok(code)) return NAF_GPU_EARG;
    for (u32 i = 0; i < 4096; i++) {
        const u32 cd[3] = { i >> 8, (i >> 4) & 15u, i & 15u };
        const u32 gaps = (cd[0] == 0) + (cd[1] == 0) + (cd[2] == 0);
        if (gaps) { lut[i] = gaps == 3 ? '-' : 'X'; continue; }
        char letter = 0;
        for (u32 a = 0; a < 4; a++) for (u32 b = 0; b < 4; b++) for (u32 d = 0; d < 4; d++)      // base x of ACGT is bit 3 - x of a code
            if ((cd[0] & (8u >> a)) && (cd[1] & (8u >> b)) && (cd[2] & (8u >> d))) {
                const char l = code->aa[16 * a + 4 * b + d];
                letter = !letter || letter == l ? l : 'X';
            }
        lut[i] = (u8)letter;
    }
    return 0;
}

// The two tables of the kernel from the contract's: [v] for the field v = c0 | c1 << 4 | c2 << 8 of a forward codon, [4096 + v] for the same
// field read as a reverse codon -- comp(c2) comp(c1) comp(c0), the complement of a code being its four bits reversed.
static void tr_kernel_tables(const u8 lut[4096], u8 tab[8192])
{
    auto rev4 = [](u32 k) { return ((k & 1u) << 3) | ((k & 2u) << 1) | ((k & 4u) >> 1) | (k >> 3); };
    for (u32 v = 0; v < 4096; v++) {
        const u32 c0 = v & 15u, c1 = (v >> 4) & 15u, c2 = v >> 8;
        tab[v] = lut[(c0 << 8) | (c1 << 4) | c2];
        tab[4096 + v] = lut[(rev4(c2) << 8) | (rev4(c1) << 4) | rev4(c0)];
    }
}

static int translate_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o, const naf_gpu_genetic_code *code,
                         const naf_gpu_segment *segs, const u8 *strand, size_t S, u8 *d_out, size_t out_cap, size_t *out_len, bool size_only)
{
    if (!c || !out_len) return NAF_GPU_EARG;
    *out_len = 0;
    if (!o) return NAF_GPU_EARG;
    u8 lut[4096];
    if (naf_gpu_codon_lut(code, lut)) return ctx_fail(c, NAF_GPU_EARG, "translate: the genetic code is NULL or holds a byte that is neither a letter A..Z nor '*'");
    const naf_gpu_unnaf_opts fasta = { NAF_OUT_FASTA, 0, o->line_length };       // FASTA-shaped whatever the archive; the mask is not decoded
    return select_run(c, d_naf, naf_len, &fasta, segs, strand, S, d_out, out_cap, out_len, size_only, false, 3, [&](naf_gpu_ctx *c, const SelCall &k) -> int {
        std::vector<u8> tab(8192);
        tr_kernel_tables(lut, tab.data());
        const size_t tb = k.any_rc ? 8192 : 4096;
        u8 *d_tab = (u8 *)arena_alloc(c, tb); if (!d_tab) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemcpyAsync(d_tab, tab.data(), tb, hipMemcpyHostToDevice, c->stream));
        const u32 grid = cdiv(k.total, 4096 * TR_WAVES);
        if (k.any_rc) LAUNCH(c, "unnaf_emit_translate_rc", k_emit_translate<true>, grid, 64 * TR_WAVES, 0, k.pl.P, (const u8 *)d_tab, k.sg, k.seg_out, k.S, k.hdr_text, k.total, k.d_out);
        else LAUNCH(c, "unnaf_emit_translate", k_emit_translate<false>, grid, 64 * TR_WAVES, 0, k.pl.P, (const u8 *)d_tab, k.sg, k.seg_out, k.S, k.hdr_text, k.total, k.d_out);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));                             // (tab, the uploaded tables, is this call's)
        if (ctx_tracing(c)) ctx_trace(c, "[translate] segments %zu codons %llu ranges %zu sequence bytes decoded %llu of %llu\n", (size_t)k.S, (unsigned long long)k.letters, k.ranges,
                                      (unsigned long long)k.decoded, (unsigned long long)k.pl.seq_bytes);
        return 0;
    });
}

extern "C" int naf_gpu_unnaf_translate_size(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o, const naf_gpu_genetic_code *code,
                                            const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len)
{
    return translate_run(c, (const u8 *)d_naf, naf_len, o, code, segs, strand, n_segs, nullptr, 0, out_len, true);
}
extern "C" int naf_gpu_unnaf_translate(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o, const naf_gpu_genetic_code *code,
                                       const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len)
{
    int rc = translate_run(c, (const u8 *)d_naf, naf_len, o, code, segs, strand, n_segs, (u8 *)d_out, out_cap, out_len, false);
    if (c) arena_settle(c);
    return rc;
}
