// emit_select.h -- the selection path of unnaf: records and regions by number, id or range (naf_gpu_unnaf_find,
// naf_gpu_unnaf_record_table, naf_gpu_unnaf_select, naf_gpu_unnaf_select_stranded, naf_gpu_unnaf_select_reads).  Part of emit.hip (included by it, behind unnaf_run): it uses that file's
// side-section chain (unnaf_prepare, unnaf_sections), the payload decode of payload.h and device helpers as they are, and adds kernels of its own.
//
// A selection is a list of SEGMENTS -- bases [begin, end) of a record -- whose texts are laid end to end in the order given.  The
// text of a segment is the text of a record that holds just those bases (header, wrapping restarted at its first base), so the
// path builds, on the device, the same tables the whole text has per record, per segment instead (k_select_layout + two scans),
// and a tile kernel composes 4 KiB of output per wavefront from them (k_emit_select).  The sequence stream is decoded only where
// the segments lie: their base intervals are sorted and merged on the host and every merged interval is one payload_range;
// every segment carries the pointers of the range that holds its bases (k_select_bind).
//
// A segment may be asked for as its REVERSE COMPLEMENT (naf_gpu_unnaf_select_stranded): the same record text with the bases read from
// end - 1 down to begin and complemented, "/rc" behind the id.  In the code table "-TGKCYSBAWRDMHVN" the complement of a code is the
// code with its four bits reversed, so the complement is a second 16-entry table (P.lutc) through the same expand16; the chunk
// composer loads the 16 forward bases (or quality bytes) that end where the chunk begins, expands and masks them at their forward
// positions -- a base keeps its own case -- and turns the 16 bytes round in registers (k_emit_select<true, true>, launched only for a
// call that holds such a segment).  Everything on the host, the decoded blocks among it, is the same for both strands.
//
// The same front serves the translation (translate.h: naf_gpu_unnaf_translate): select_run takes the bases to a byte of the body (1, or 3 for
// amino acids) and the launch of the kernel that writes the text; everything in front of that launch is one code for both.
//
// A selection of READS (naf_gpu_unnaf_select_reads: trimmed reads) differs in one thing: a sub-range keeps the header line of its whole
// record (SEL_READ in place of SEL_SUB), and so has a FASTQ form -- the composer takes bases and qualities from g0 / n of any segment.
#pragma once
#include <algorithm>

#define SEL_MAX_RANGES 32                    // separately decoded ranges of a call; beyond it the merge gap doubles until they fit
#define SEL_GAP_BLOCKS 2                     // neighbours no further apart than this many 128 KiB blocks of stream are decoded as one

struct SelSeg {
    u64 g0, n;                               // first base (index in the archive's sequence stream) and number of bases
    u64 ho;                                  // its header line in the header stream
    u64 klo, khi;                            // mask toggles that can fall inside it: toggles[klo .. khi)
    u64 rec, begin;                          // record and 0-based first base inside it
    const u8 *seq, *qual;                    // the decoded range that holds its bases, as pointers to stream byte 0 / quality byte 0
    u32 hl, sub;                             // header length; SEL_SUB = a sub-range (header '>' id ':' begin+1 '-' end), SEL_RC = reverse complement ("/rc" behind it), SEL_READ = a sub-range under its record's own header
};
#define SEL_SUB 1u
#define SEL_RC 2u
#define SEL_READ 4u
struct SelRange { u64 g_lo, g_hi; const u8 *seq, *qual; };

__device__ __forceinline__ u32 dec_digits(u64 v) { u32 n = 1; while (v >= 10) { v /= 10; n++; } return n; }

// One lane per segment: validation, geometry, text size.  status[0] receives the number of the first segment that cannot be
// produced (atomicMin; ~0 = none).  size[] / hsize[] are scanned into the text offsets and the header stream offsets.
// per: bases per byte of the body, 1 for the bases themselves, 3 for their translation (translate.h; FASTA only): the wrap counts the bytes.
// reads: a sub-range is a read cut short -- its record's header line, FASTQ allowed.
__global__ __launch_bounds__(256) void k_select_layout(EmitP P, const naf_gpu_segment *in, const u8 *strand, u64 S, u32 per, u32 reads, SelSeg *sg, u64 *size, u64 *hsize, u64 *iv, unsigned long long *status)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const u64 rec = in[s].record, b = in[s].begin; u64 e = in[s].end;
    const bool whole = b == 0 && e == ~0ull, rc = strand && strand[s];          // (strand: nullptr when the call has no reverse segment)
    SelSeg g; memset(&g, 0, sizeof g);
    bool bad = rec >= P.N;
    u64 len = 0;
    if (!bad) { len = P.rec_len[rec]; if (e > len) e = len; bad = !whole && (b >= e || (P.mode == EM_FASTQ && !reads)); }
    if (bad) { atomicMin(status, (unsigned long long)s); size[s] = 0; hsize[s] = 0; iv[2 * s] = iv[2 * s + 1] = 0; sg[s] = g; return; }
    g.rec = rec; g.begin = whole ? 0 : b; g.n = whole ? len : e - b; g.g0 = P.rec_base[rec] + g.begin; g.sub = (whole ? 0u : reads ? SEL_READ : SEL_SUB) | (rc ? SEL_RC : 0u);
    u64 h = 0;
    if (P.mode == EM_FASTA || P.mode == EM_FASTQ) {
        if (whole || reads) h = P.hdr_len[rec];
        else { const u64 idl = P.has_ids ? P.idz[rec] - (rec ? P.idz[rec - 1] + 1 : 0) : 0; h = 1 + idl + 1 + dec_digits(b + 1) + 1 + dec_digits(e) + 1; }
        if (rc) h += 3;                                                           // "/rc"
    }
    g.hl = (u32)h;
    u64 body;
    if (P.mode == EM_FASTQ) body = 2 * g.n + 4;
    else if (P.mode == EM_SEQUENCES) body = g.n + 1;
    else if (P.mode == EM_SEQ) body = g.n;
    else { const u64 nb = per == 1 ? g.n : g.n / per; body = nb ? nb + (P.L ? (nb + P.L - 1) / P.L : 1) : 0; }   // as rec_size_of
    if (P.masking) { g.klo = upper_bound_u64(P.toggles, 0, P.n_toggles, g.g0); g.khi = upper_bound_u64(P.toggles, g.klo, P.n_toggles, g.g0 + g.n); }
    size[s] = h + body; hsize[s] = h;
    iv[2 * s] = g.g0; iv[2 * s + 1] = g.g0 + g.n;
    sg[s] = g;
}

// Header lines of the segments as one byte stream, eight lanes per segment (k_hdr_build's shape): a whole record's line from its id
// and name, a sub-range's from its id and the two numbers; "/rc" directly behind the id (behind the range; behind the name of an archive
// without ids) for a reverse segment.
__global__ __launch_bounds__(256) void k_select_hdr(EmitP P, SelSeg *sg, u64 S, const u64 *hoff, u8 *text)
{
    const u64 s = (u64)blockIdx.x * 32 + (threadIdx.x >> 3);
    const u32 g = threadIdx.x & 7;
    if (s >= S) return;
    const u64 r = sg[s].rec; const u32 hl = sg[s].hl, rc = sg[s].sub & SEL_RC ? 3u : 0u;
    if (g == 0) sg[s].ho = hoff[s];
    if (!hl) return;
    u8 *o = text + hoff[s];
    u64 ids0 = 0, idl = 0, nm0 = 0, nml = 0;
    if (P.has_ids) { ids0 = r ? P.idz[r - 1] + 1 : 0; idl = P.idz[r] - ids0; }
    if (P.has_names) { nm0 = r ? P.nmz[r - 1] + 1 : 0; nml = P.nmz[r] - nm0; }
    if (g == 0) { o[0] = P.hdr_char; o[hl - 1] = '\n'; }
    if (sg[s].sub & SEL_SUB) {
        if (P.has_ids) group_copy<8>(o + 1, P.ids + ids0, idl, g);
        if (g == 0) {                                                             // ':' a '-' b, written backwards from the line's end
            u8 *q = o + hl - 1;
            if (rc) { *--q = 'c'; *--q = 'r'; *--q = '/'; }
            u64 v = sg[s].begin + sg[s].n; do { *--q = (u8)('0' + v % 10); v /= 10; } while (v);
            *--q = '-';
            v = sg[s].begin + 1; do { *--q = (u8)('0' + v % 10); v /= 10; } while (v);
            *--q = ':';
        }
    } else if (P.has_ids) {
        group_copy<8>(o + 1, P.ids + ids0, idl, g);
        if (rc && g == 0) { o[1 + idl] = '/'; o[2 + idl] = 'r'; o[3 + idl] = 'c'; }
        if (P.has_names && nml) { if (g == 0) o[1 + idl + rc] = P.sep; group_copy<8>(o + 2 + idl + rc, P.names + nm0, nml, g); }
    } else {
        group_copy<8>(o + 1, P.names + nm0, nml, g);
        if (rc && g == 0) { o[hl - 4] = '/'; o[hl - 3] = 'r'; o[hl - 2] = 'c'; }
    }
}

// Every segment takes the pointers of the decoded range that holds its bases (ranges sorted by g_lo, disjoint).
__global__ __launch_bounds__(256) void k_select_bind(SelSeg *sg, u64 S, const SelRange *rg, u32 R)
{
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= S || !R) return;
    const u64 g0 = sg[s].g0;
    u32 lo = 0, hi = R;                                                           // last range with g_lo <= g0
    while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (rg[mid].g_lo <= g0) lo = mid; else hi = mid; }
    sg[s].seq = rg[lo].seq; sg[s].qual = rg[lo].qual;
}

// 16 bases from base index g of the stream at `seq` (bases16 without the flat-frame source, which this path never has)
template <bool FOURBIT>
__device__ __forceinline__ void sel_bases16(const EmitP &P, const u32 lut[4], const u8 *seq, u64 g, u64 &lo, u64 &hi)
{
    if (!FOURBIT) {
        lo = ld64(seq + g); hi = ld64(seq + g + 8);
        if (P.upper) {
            auto up = [](u64 v) { u64 r = 0; for (int i = 0; i < 8; i++) { u32 c = (v >> (8 * i)) & 0xFF; if (c >= 'a' && c <= 'z') c -= 32; r |= (u64)c << (8 * i); } return r; };
            lo = up(lo); hi = up(hi);
        }
        return;
    }
    const u8 *a = seq + (g >> 1);
    u64 nib = ld64(a);
    if (g & 1) nib = (nib >> 4) | ((u64)a[8] << 60);                               // a region that starts on a low nibble
    expand16(lut, nib, lo, hi);
}

// The first c (1 .. 16) bytes of {lo,hi} in reverse order, from byte 0 on: all sixteen turned round, the 16 - c that do not belong
// shifted out.
__device__ __forceinline__ void reverse16(u64 &lo, u64 &hi, u32 c)
{
    u64 a = __builtin_bswap64(hi), b = __builtin_bswap64(lo);
    const u32 sh = 8 * (16 - c);
    if (sh >= 64) { a = b >> (sh - 64); b = 0; } else if (sh) { a = (a >> sh) | (b << (64 - sh)); b >>= sh; }
    lo = a; hi = b;
}

// One 16-byte chunk of the selection's text, composed piece by piece as compose_chunk composes a chunk of the whole text: a piece
// is n_main bytes of header, bases or qualities followed by up to three constant bytes.  s: the segment that holds byte p0.
// RC: the call holds reverse segments.  Output base j of one is stream base g0 + len - 1 - j, so a piece that starts at base j takes
// the c = min(16, len - j) bases that end there -- one forward load from g0 + len - j - c, which never starts before the segment and
// reads past the piece no further than a forward piece does -- complemented by the table, masked where they stand, then reversed.
// The qualities of a reverse read likewise.
template <bool FOURBIT, bool RC>
__device__ __forceinline__ void select_chunk(const EmitP &P, const SelSeg *sg, const u64 *seg_out, const u8 *hdr_text, u64 p0, u32 nbytes, u64 s, u32 Lp1_32, u8 *o)
{
    u64 so = seg_out[s], sn = seg_out[s + 1];
    SelSeg g = sg[s];
    u64 lo = 0, hi = 0; u32 pos = 0;
    while (pos < nbytes) {
        const u64 p = p0 + pos;
        while (p >= sn) { s++; so = sn; sn = seg_out[s + 1]; g = sg[s]; }            // (p < seg_out[S]: the loop ends inside the table)
        const u64 off = p - so, len = g.n;
        const u8 *src = nullptr; u64 gi = 0; bool is_bases = false;
        u64 n_main = 0; u32 tc = 0, n_tc = 0;
        u32 rc_c = 0;                                                             // RC: source bytes to reverse into this piece (0: a forward piece)
        if (off < g.hl) { src = hdr_text + g.ho + off; n_main = g.hl - off; }
        else {
            const u64 q = off - g.hl;
            if (P.mode == EM_FASTQ) {
                if (q < len + 3) {
                    u64 skip = 0;
                    if (q < len) { is_bases = true; gi = g.g0 + q; n_main = len - q; } else skip = q - len;
                    tc = 0x0A2B0Au >> (8 * (u32)skip); n_tc = 3 - (u32)skip;
                } else {
                    src = g.qual + g.g0 + (q - len - 3); n_main = 2 * len + 3 - q; tc = '\n'; n_tc = 1;
                    if (RC && (g.sub & SEL_RC)) { rc_c = n_main < 16 ? (u32)n_main : 16u; src = g.qual + g.g0 + n_main - rc_c; }
                }
            } else if (P.mode == EM_SEQ) { is_bases = true; gi = g.g0 + q; n_main = len - q; }
            else {
                tc = '\n'; n_tc = 1;
                if (P.mode == EM_SEQUENCES || P.L == 0) { if (q < len) { is_bases = true; gi = g.g0 + q; n_main = len - q; } }
                else {
                    u64 line, col;
                    if (Lp1_32 && (q >> 32) == 0) { const u32 l32 = (u32)q / Lp1_32; line = l32; col = (u32)q - l32 * Lp1_32; }
                    else { line = q / (P.L + 1); col = q - line * (P.L + 1); }
                    const u64 j = line * P.L + col;
                    if (col != P.L && j < len) { is_bases = true; gi = g.g0 + j; n_main = len - j < P.L - col ? len - j : P.L - col; }
                }
            }
        }
        u32 rem = nbytes - pos;
        const u32 n1 = n_main < rem ? (u32)n_main : rem;
        if (n1) {
            u64 slo, shi;
            if (is_bases) {
                if (RC && (g.sub & SEL_RC)) {
                    const u64 left = g.g0 + len - gi;                             // bases of the segment from this output base on
                    rc_c = left < 16 ? (u32)left : 16u; gi = g.g0 + left - rc_c;
                    const u32 lc[4] = { P.lutc[0], P.lutc[1], P.lutc[2], P.lutc[3] };
                    sel_bases16<FOURBIT>(P, lc, g.seq, gi, slo, shi);
                }
                else sel_bases16<FOURBIT>(P, P.lut, g.seq, gi, slo, shi);
                if (P.masking) {
                    u64 klo = g.klo, khi = g.khi;
                    if (khi - klo > 0x7FFFFFFFull) { klo = upper_bound_u64(P.toggles, klo, khi, gi); if (khi - klo > 17) khi = klo + 17; }   // at most 16 toggles inside 16 bases
                    if (klo < khi) mask16_from(P.toggles + klo, (u32)(khi - klo), klo, gi, slo, shi);
                    else if (klo & 1) { slo += 0x2020202020202020ull; shi += 0x2020202020202020ull; }
                }
            }
            else { slo = ld64(src); shi = (RC && rc_c ? rc_c : n1) > 8 ? ld64(src + 8) : 0; }
            if (RC && rc_c) reverse16(slo, shi, rc_c);
            place16(lo, hi, slo, shi, pos, n1);
            pos += n1; rem -= n1;
        }
        if (n1 == n_main && rem && n_tc) { const u32 n2 = n_tc < rem ? n_tc : rem; place16(lo, hi, tc, 0, pos, n2); pos += n2; }
    }
    store_upto16(o, lo, hi, nbytes);
}

// One wavefront per 4 KiB tile of the output, four rounds of 64 lanes x 16 bytes: a round is one KiB of consecutive 16-byte stores.
// The tile's first and last segment are found once (the same in every lane: scalar loads); a lane searches between them only when
// the tile spans several segments (short reads: ~300 bytes of text each).
// RC = true is the instantiation of a call with reverse segments (4-bit streams only); a call without one runs <FOURBIT, false>.
template <bool FOURBIT, bool RC = false>
__global__ __launch_bounds__(64) void k_emit_select(EmitP P, const SelSeg *sg, const u64 *seg_out, u64 S, const u8 *hdr_text, u64 total, u8 *out)
{
    const u64 t0 = (u64)xcd_block() * 4096, t1 = t0 + 4096 < total ? t0 + 4096 : total;
    if (t0 >= total) return;
    const u64 s_lo = upper_bound_u64(seg_out, 0, S + 1, t0) - 1, s_hi = upper_bound_u64(seg_out, s_lo, S + 1, t1 - 1) - 1;
    const u32 Lp1_32 = (P.L + 1) >> 32 ? 0 : (u32)(P.L + 1);
#pragma unroll 1
    for (u32 k = 0; k < 4; k++) {
        const u64 p0 = t0 + k * 1024 + threadIdx.x * 16;
        if (p0 >= t1) break;
        const u32 nbytes = t1 - p0 < 16 ? (u32)(t1 - p0) : 16u;
        const u64 s = s_lo == s_hi ? s_lo : upper_bound_u64(seg_out, s_lo, s_hi + 1, p0) - 1;
        select_chunk<FOURBIT, RC>(P, sg, seg_out, hdr_text, p0, nbytes, s, Lp1_32, out + p0);
    }
}

// ---- ids -> record numbers -----------------------------------------------------------------------------------------------------
// What the table is probed with: the length, the first 16 and the last 16 bytes of an id -- a fixed amount of work per id whatever
// its length (read names differ at their ends, accession numbers at either).  p must be readable for 16 bytes from its start.
NAF_HD u64 id_hash(const u8 *p, u64 len)
{
    u64 w[4] = { 0, 0, 0, 0 };
    if (len >= 16) { w[0] = ld64(p); w[1] = ld64(p + 8); w[2] = ld64(p + len - 16); w[3] = ld64(p + len - 8); }
    else {
        const u64 a = ld64(p), b = ld64(p + 8);
        w[0] = len >= 8 ? a : (a & ((1ull << (8 * len)) - 1));
        w[1] = len > 8 ? (b & ((1ull << (8 * (len - 8))) - 1)) : 0;
    }
    u64 h = (len + 1) * 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 4; i++) { h = (h ^ w[i]) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    return h;
}
#define FIND_LOCAL 32u                        // ids up to this length are compared by their own lane; longer ones by the wavefront, 1 KiB a step
__device__ __forceinline__ u64 shfl_u64(u64 v, int src) { return ((u64)(u32)__shfl((int)(v >> 32), src) << 32) | (u32)__shfl((int)(u32)v, src); }
// n (<= 16) bytes at a and b differ?  Both readable for 16 bytes.
__device__ __forceinline__ bool differ16(const u8 *a, const u8 *b, u32 n)
{
    u64 x = ld64(a) ^ ld64(b), y = ld64(a + 8) ^ ld64(b + 8);
    if (n < 8) { x &= (1ull << (8 * n)) - 1; y = 0; } else if (n < 16) y &= (1ull << (8 * (n - 8))) - 1;
    return (x | y) != 0;
}
// A lane per record: hash of its id, probe of the open-addressing table of the queries (entry: query number + 1 in the low word,
// the upper word of the query's hash above it; 0 = empty), byte comparison on a hit, 64-bit atomicMin of the record number into
// records[query] -- the first record in archive order wins whatever the scheduling.  Queries that repeat sit in the table once each.
__global__ __launch_bounds__(64) void k_find_ids(const u8 *ids, const u64 *idz, u64 N, const u64 *table, u32 tmask, const u8 *qb, const u64 *qoff, unsigned long long *records)
{
    const u32 lane = threadIdx.x;
    const u64 r = (u64)blockIdx.x * 64 + lane;
    u64 s0 = 0, len = 0, h = 0; u32 slot = 0;
    bool probing = r < N;
    if (probing) { s0 = r ? idz[r - 1] + 1 : 0; len = idz[r] - s0; h = id_hash(ids + s0, len); slot = (u32)h & tmask; }
    while (__any(probing)) {
        const u64 e = probing ? table[slot] : 0;
        if (e == 0) probing = false;
        bool cand = probing && (u32)(e >> 32) == (u32)(h >> 32);
        const u32 q = (u32)e - 1;
        u64 q0 = 0;
        if (cand) { q0 = qoff[q]; cand = qoff[q + 1] - q0 - 1 == len; }
        if (cand && len <= FIND_LOCAL) {
            bool d = false;
            for (u32 k = 0; k < (u32)len; k += 16) d = d || differ16(ids + s0 + k, qb + q0 + k, (u32)len - k < 16 ? (u32)len - k : 16u);
            if (!d) atomicMin(&records[q], (unsigned long long)r);
            cand = false;
        }
        u64 pend = __ballot(cand);
        while (pend) {                                                                // a long id: the whole wavefront compares it
            const int src = __ffsll((unsigned long long)pend) - 1; pend &= pend - 1;
            const u64 a0 = shfl_u64(s0, src), b0 = shfl_u64(q0, src), n = shfl_u64(len, src);
            bool d = false;
            for (u64 k = (u64)lane * 16; k < n; k += 1024) d = d || differ16(ids + a0 + k, qb + b0 + k, n - k < 16 ? (u32)(n - k) : 16u);
            if (!__any(d) && (int)lane == src) atomicMin(&records[q], (unsigned long long)r);
        }
        if (probing) slot = (slot + 1) & tmask;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_parse_region(const char *text, size_t *id_len, uint64_t *begin, uint64_t *end)
{
    if (!text || !id_len || !begin || !end) return NAF_GPU_EARG;
    const size_t n = strlen(text);
    *id_len = n; *begin = 0; *end = NAF_GPU_WHOLE;
    if (n == 0) return NAF_GPU_EARG;
    const char *colon = strrchr(text, ':');
    if (!colon) return 0;
    const char *p = colon + 1;
    if (!*p || strspn(p, "0123456789,-") != strlen(p)) return 0;              // not a range: the ':' belongs to the id
    if (colon == text) return NAF_GPU_EARG;                                    // a range of nothing
    auto number = [&](uint64_t *v) -> bool {                                   // digits with commas among them
        uint64_t a = 0; int nd = 0;
        if (*p == ',') return false;
        for (; (*p >= '0' && *p <= '9') || *p == ','; p++) {
            if (*p == ',') continue;
            if (a > (UINT64_MAX - 9) / 10) return false;
            a = a * 10 + (uint64_t)(*p - '0'); nd++;
        }
        *v = a; return nd > 0;
    };
    uint64_t a = 0, b = 0;
    if (!number(&a) || a == 0) return NAF_GPU_EARG;
    if (!*p) b = a;                                                            // ID:a -- one base
    else {
        if (*p++ != '-') return NAF_GPU_EARG;
        if (!*p) b = NAF_GPU_WHOLE;                                            // ID:a- -- to the record's end
        else if (!number(&b) || *p || b < a) return NAF_GPU_EARG;
    }
    *id_len = (size_t)(colon - text); *begin = a - 1; *end = b;
    return 0;
}

extern "C" int naf_gpu_unnaf_find(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const char *h_ids, size_t ids_bytes, size_t n_ids, uint64_t *records)
{
    if (!c || !d_naf || (n_ids && (!h_ids || !records))) return NAF_GPU_EARG;
    arena_reset(c);
    // the queries: offsets of the strings (each with its terminator)
    std::vector<u64> qoff(n_ids + 1);
    { size_t at = 0;
      for (size_t k = 0; k < n_ids; k++) {
          const void *z = at < ids_bytes ? memchr(h_ids + at, 0, ids_bytes - at) : nullptr;
          if (!z) return ctx_fail(c, NAF_GPU_EARG, "find: %zu ids announced, %zu zero-terminated strings in %zu bytes", n_ids, k, ids_bytes);
          qoff[k] = at; at = (size_t)((const char *)z - h_ids) + 1;
      }
      qoff[n_ids] = at; }
    naf_gpu_unnaf_opts o = { NAF_OUT_FASTA, 0, -1 };
    UnnafPlan pl;
    int rc = unnaf_prepare(c, (const u8 *)d_naf, naf_len, &o, pl); if (rc) return rc;
    const naf_gpu_header &h = pl.h;
    if (!((h.flags >> 5) & 1)) return ctx_fail(c, NAF_GPU_EARG, "find: the archive stores no ids");
    for (size_t k = 0; k < n_ids; k++) records[k] = UINT64_MAX;
    const u64 N = h.n_sequences;
    if (!n_ids || !N) return 0;
    if (n_ids >= 0x7FFFFFFFull) return ctx_fail(c, NAF_GPU_EARG, "find: too many ids in one call");
    if (h.orig_size[S_IDS] == 0) return ctx_fail(c, NAF_GPU_EFORMAT, "corrupted ids - not 0-terminated\n");
    u8 *ids = nullptr; u64 *idz = nullptr;
    if ((rc = load_section(c, (const u8 *)d_naf, h, S_IDS, h.orig_size[S_IDS], "ids", &ids, pl.frame_head[S_IDS]))) return rc;
    if ((rc = zero_positions(c, ids, h.orig_size[S_IDS], N, &idz, false))) return rc;
    // the table of the queries, at most half full
    u64 slots = 16; while (slots < 2 * (u64)n_ids) slots <<= 1;
    std::vector<u64> table(slots, 0);
    std::vector<u8> qb(qoff[n_ids] + 32, 0);
    memcpy(qb.data(), h_ids, qoff[n_ids]);
    for (size_t k = 0; k < n_ids; k++) {
        const u64 hq = id_hash(qb.data() + qoff[k], qoff[k + 1] - qoff[k] - 1);
        u64 s = (u32)hq & (slots - 1);
        while (table[s]) s = (s + 1) & (slots - 1);
        table[s] = (hq & 0xFFFFFFFF00000000ull) | (u64)(k + 1);
    }
    u64 *d_table = arena_new<u64>(c, slots), *d_qoff = arena_new<u64>(c, n_ids + 1);
    u8 *d_qb = (u8 *)arena_alloc(c, qb.size());
    unsigned long long *d_rec = arena_new<unsigned long long>(c, n_ids);
    if (!d_table || !d_qoff || !d_qb || !d_rec) return NAF_GPU_ENOMEM;
    HIP_TRY(c, hipMemcpyAsync(d_table, table.data(), slots * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_qoff, qoff.data(), (n_ids + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_qb, qb.data(), qb.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_rec, 0xFF, n_ids * 8, c->stream));
    LAUNCH(c, "unnaf_find_ids", k_find_ids, cdiv(N, 64), 64, 0, (const u8 *)ids, (const u64 *)idz, N, (const u64 *)d_table, (u32)(slots - 1), (const u8 *)d_qb, (const u64 *)d_qoff, d_rec);
    HIP_TRY(c, hipMemcpyAsync(records, d_rec, n_ids * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    arena_settle(c);
    return 0;
}

// prepare + side sections for a call that addresses records: --seq has no record tables of its own (its text is the base stream), so
// they are made as for --sequences and the mode is put back
static int select_tables(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o, UnnafPlan &pl)
{
    int rc = unnaf_prepare(c, d_naf, naf_len, o, pl); if (rc) return rc;
    if (pl.P.mode == -1) return ctx_fail(c, NAF_GPU_EARG, "records of the 4-bit stream cannot be selected");
    if (pl.empty) return 0;
    const int mode = pl.P.mode;
    if (mode == EM_SEQ) pl.P.mode = EM_SEQUENCES;
    rc = unnaf_sections(c, d_naf, pl);
    pl.P.mode = mode;
    return rc;
}

extern "C" int naf_gpu_unnaf_record_table(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                          uint64_t first, uint64_t count, uint64_t *n_bases, uint64_t *text_off)
{
    if (!c || !d_naf || !o || !text_off) return NAF_GPU_EARG;
    arena_reset(c);
    UnnafPlan pl;
    int rc = select_tables(c, (const u8 *)d_naf, naf_len, o, pl); if (rc) return rc;
    const u64 N = pl.h.n_sequences;
    if (first > N || count > N - first) return ctx_fail(c, NAF_GPU_EARG, "record table: records %llu..%llu of %llu", (unsigned long long)first, (unsigned long long)(first + count), (unsigned long long)N);
    if (pl.empty) { for (u64 k = 0; k <= count; k++) text_off[k] = 0; if (n_bases) for (u64 k = 0; k < count; k++) n_bases[k] = 0; return 0; }
    const u64 *off = pl.P.mode == EM_SEQ ? pl.P.rec_base : pl.P.rec_out;
    HIP_TRY(c, hipMemcpyAsync(text_off, off + first, (count + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_bases && count) HIP_TRY(c, hipMemcpyAsync(n_bases, pl.P.rec_len + first, count * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    arena_settle(c);
    return 0;
}

// What the kernel that writes a selection's text is launched with: the tables select_run made, every segment bound to its decoded range.
struct SelCall {
    UnnafPlan &pl; const SelSeg *sg; const u64 *seg_out; u64 S; const u8 *hdr_text; u64 total; u8 *d_out;
    bool any_rc; size_t ranges; u64 decoded, letters;                            // letters: the sum of floor(bases / per) over the segments
};
// The text of naf_gpu_unnaf_select: the bases (or bytes) themselves
static int select_emit(naf_gpu_ctx *c, const SelCall &k)
{
    const EmitP &P = k.pl.P;
    const u32 grid = cdiv(k.total, 4096);
    if (k.any_rc) LAUNCH(c, "unnaf_emit_select_rc", (k_emit_select<true, true>), grid, 64, 0, P, k.sg, k.seg_out, k.S, k.hdr_text, k.total, k.d_out);
    else if (k.pl.fourbit) LAUNCH(c, "unnaf_emit_select", k_emit_select<true>, grid, 64, 0, P, k.sg, k.seg_out, k.S, k.hdr_text, k.total, k.d_out);
    else LAUNCH(c, "unnaf_emit_select", k_emit_select<false>, grid, 64, 0, P, k.sg, k.seg_out, k.S, k.hdr_text, k.total, k.d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));                                 // (the uploaded range table is this call's)
    if (ctx_tracing(c)) ctx_trace(c, "[select] segments %zu ranges %zu sequence bytes decoded %llu of %llu side sections 1\n", (size_t)k.S, k.ranges, (unsigned long long)k.decoded, (unsigned long long)k.pl.seq_bytes);
    return 0;
}

// h_strand: one byte per segment, 1 = its reverse complement; nullptr = none.  per, emit: 1 and select_emit; 3 and translate.h's for the
// translation, which is FASTA-shaped whatever the archive and needs a 4-bit stream.  reads: naf_gpu_unnaf_select_reads (sub-ranges under their record's header).
template <typename Emit>
static int select_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o, const naf_gpu_segment *h_segs, const u8 *h_strand, size_t S,
                      u8 *d_out, size_t out_cap, size_t *out_len, bool size_only, bool reads, u32 per, Emit emit)
{
    if (!c || !d_naf || !o || !out_len || (S && !h_segs)) return NAF_GPU_EARG;
    arena_reset(c);
    *out_len = 0;
    size_t first_rc = S;
    if (h_strand) for (size_t k = 0; k < S; k++) {
        if (h_strand[k] > 1) return ctx_fail(c, NAF_GPU_EARG, "segment %zu: strand %u is neither 0 (as stored) nor 1 (reverse complement)", k, (unsigned)h_strand[k]);
        if (h_strand[k] && first_rc == S) first_rc = k;
    }
    const bool any_rc = first_rc < S;
    UnnafPlan pl;
    int rc = select_tables(c, d_naf, naf_len, o, pl); if (rc) return rc;
    if (per != 1) {
        if (!pl.fourbit) return ctx_fail(c, NAF_GPU_EARG, "translate: %s sequences cannot be translated", pl.h.seq_type == NAF_SEQ_PROTEIN ? "protein" : "text");
        if (!((pl.h.flags >> 1) & 1)) return ctx_fail(c, NAF_GPU_EARG, "translate: the archive stores no sequence");
    }
    if (any_rc && !pl.fourbit) return ctx_fail(c, NAF_GPU_EARG, "segment %zu: a %s sequence has no reverse complement", first_rc, pl.h.seq_type == NAF_SEQ_PROTEIN ? "protein" : "text");
    if (S == 0) return 0;
    const naf_gpu_header &h = pl.h;
    EmitP &P = pl.P;
    if (pl.empty) {                                                              // no records, or records without data: the whole text is empty
        if (h.n_sequences == 0) return ctx_fail(c, NAF_GPU_EARG, "segment 0: record %llu is not in the archive (0 records)", (unsigned long long)h_segs[0].record);
        return 0;
    }
    // layout: the segments' geometry and sizes, validated on the device
    naf_gpu_segment *d_in = arena_new<naf_gpu_segment>(c, S);
    SelSeg *sg = arena_new<SelSeg>(c, S + 1);
    u64 *seg_out = arena_new<u64>(c, S + 2), *hoff = arena_new<u64>(c, S + 2), *iv = arena_new<u64>(c, 2 * S);
    unsigned long long *d_status = arena_new<unsigned long long>(c, 1);
    u8 *d_strand = any_rc ? (u8 *)arena_alloc(c, S) : nullptr;
    if (!d_in || !sg || !seg_out || !hoff || !iv || !d_status || (any_rc && !d_strand)) return NAF_GPU_ENOMEM;
    if (any_rc) HIP_TRY(c, hipMemcpyAsync(d_strand, h_strand, S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_in, h_segs, S * sizeof *h_segs, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_status, 0xFF, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(seg_out + S, 0, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(hoff + S, 0, 8, c->stream));
    LAUNCH(c, "unnaf_select_layout", k_select_layout, cdiv(S, 256), 256, 0, P, (const naf_gpu_segment *)d_in, (const u8 *)d_strand, (u64)S, per, reads ? 1u : 0u, sg, seg_out, hoff, iv, d_status);
    if ((rc = scan_exclusive_u64(c, seg_out, S + 1, (u64 *)nullptr))) return rc;
    if ((rc = scan_exclusive_u64(c, hoff, S + 1, (u64 *)nullptr))) return rc;
    u64 first_bad = 0, total = 0, htotal = 0;
    { void *hp[3] = { &first_bad, &total, &htotal }; const void *dp[3] = { d_status, seg_out + S, hoff + S }; const size_t nb[3] = { 8, 8, 8 };
      if ((rc = ctx_readbackv(c, 3, hp, dp, nb))) return rc; }
    if (first_bad != ~0ull) {
        const naf_gpu_segment &sgm = h_segs[first_bad];
        if (sgm.record >= P.N) return ctx_fail(c, NAF_GPU_EARG, "segment %llu: record %llu is not in the archive (%llu records)", (unsigned long long)first_bad, (unsigned long long)sgm.record, (unsigned long long)P.N);
        if (P.mode == EM_FASTQ && !reads) return ctx_fail(c, NAF_GPU_EARG, "segment %llu: a part of a record (bases %llu..%llu of record %llu) has no FASTQ form", (unsigned long long)first_bad, (unsigned long long)sgm.begin, (unsigned long long)sgm.end, (unsigned long long)sgm.record);
        u64 len = 0; if ((rc = ctx_readback(c, &len, P.rec_len + sgm.record, 8))) return rc;
        return ctx_fail(c, NAF_GPU_EARG, "segment %llu: bases %llu..%llu select nothing of record %llu (%llu bases)", (unsigned long long)first_bad, (unsigned long long)sgm.begin, (unsigned long long)sgm.end, (unsigned long long)sgm.record, (unsigned long long)len);
    }
    if (P.mode == EM_SEQUENCES && P.T == 0) total = 0;                           // output-sequences.c:81: nothing printed
    *out_len = total;
    if (size_only || total == 0) return 0;
    if (total > out_cap) return ctx_fail(c, NAF_GPU_ECAP, "unnaf selection needs %llu bytes, capacity %zu", (unsigned long long)total, out_cap);
    if (!d_out) return NAF_GPU_EARG;
    u8 *hdr_text = (u8 *)arena_alloc(c, htotal + 32); if (!hdr_text) return NAF_GPU_ENOMEM;
    LAUNCH(c, "unnaf_select_hdr", k_select_hdr, cdiv(S, 32), 256, 0, P, sg, (u64)S, (const u64 *)hoff, hdr_text);
    // the base intervals, sorted and merged: neighbours whose gap is at most SEL_GAP_BLOCKS blocks of stream become one range
    std::vector<std::pair<u64, u64>> ivs(S);
    HIP_TRY(c, hipMemcpyAsync(ivs.data(), iv, S * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    u64 letters = 0;
    { size_t k = 0; for (size_t i = 0; i < S; i++) { letters += (ivs[i].second - ivs[i].first) / per; if (ivs[i].second > ivs[i].first) ivs[k++] = ivs[i]; } ivs.resize(k); }
    std::sort(ivs.begin(), ivs.end());
    const u64 per_byte = pl.fourbit ? 2 : 1;
    std::vector<std::pair<u64, u64>> rgs;
    for (u64 gap = (u64)SEL_GAP_BLOCKS * 131072 * per_byte; ; gap *= 2) {
        rgs.clear();
        for (const auto &x : ivs) { if (!rgs.empty() && x.first <= rgs.back().second + gap) { if (x.second > rgs.back().second) rgs.back().second = x.second; } else rgs.push_back(x); }
        if (rgs.size() <= SEL_MAX_RANGES) break;
    }
    std::vector<SelRange> hr(rgs.size());
    u64 decoded = 0;
    bool whole_stream = false;
    PayloadSpan sp, qp;
    for (size_t k = 0; k < rgs.size() && !whole_stream; k++) {
        const u64 g_lo = rgs[k].first, g_hi = rgs[k].second;
        rc = payload_range(c, d_naf, pl, S_SEQ, g_lo / per_byte, (g_hi + per_byte - 1) / per_byte, PAYLOAD_RANGE_ONLY, &sp);
        if (!rc && pl.need_qual) rc = payload_range(c, d_naf, pl, S_QUAL, g_lo, g_hi, PAYLOAD_RANGE_ONLY, &qp);
        if (rc == NAF_GPU_ECAP) { whole_stream = true; break; }                  // dependent blocks: the closure is the whole stream
        if (rc) return rc;
        hr[k] = SelRange{ g_lo, g_hi, sp.base, pl.need_qual ? qp.base : nullptr };
        decoded += sp.got_hi - sp.got_lo;
    }
    if (whole_stream) {                                                          // one decode of everything for the call, as unnaf_run does
        if ((rc = payload_range(c, d_naf, pl, S_SEQ, 0, 0, PAYLOAD_WHOLE, &sp))) return rc;
        if (pl.need_qual && (rc = payload_range(c, d_naf, pl, S_QUAL, 0, 0, PAYLOAD_WHOLE, &qp))) return rc;
        hr.assign(1, SelRange{ 0, P.T, sp.base, pl.need_qual ? qp.base : nullptr });
        decoded = pl.seq_bytes;
    }
    if (!hr.empty()) {
        SelRange *d_rg = arena_new<SelRange>(c, hr.size()); if (!d_rg) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemcpyAsync(d_rg, hr.data(), hr.size() * sizeof(SelRange), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, "unnaf_select_bind", k_select_bind, cdiv(S, 256), 256, 0, sg, (u64)S, (const SelRange *)d_rg, (u32)hr.size());
    }
    return emit(c, SelCall{ pl, sg, seg_out, (u64)S, hdr_text, total, d_out, any_rc, hr.size(), decoded, letters });
}

extern "C" int naf_gpu_unnaf_select_size(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                         const naf_gpu_segment *segs, size_t n_segs, size_t *out_len)
{
    return select_run(c, (const u8 *)d_naf, naf_len, o, segs, nullptr, n_segs, nullptr, 0, out_len, true, false, 1, select_emit);
}
extern "C" int naf_gpu_unnaf_select(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                    const naf_gpu_segment *segs, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len)
{
    int rc = select_run(c, (const u8 *)d_naf, naf_len, o, segs, nullptr, n_segs, (u8 *)d_out, out_cap, out_len, false, false, 1, select_emit);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_select_stranded_size(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                                  const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len)
{
    return select_run(c, (const u8 *)d_naf, naf_len, o, segs, strand, n_segs, nullptr, 0, out_len, true, false, 1, select_emit);
}
extern "C" int naf_gpu_unnaf_select_stranded(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                             const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len)
{
    int rc = select_run(c, (const u8 *)d_naf, naf_len, o, segs, strand, n_segs, (u8 *)d_out, out_cap, out_len, false, false, 1, select_emit);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_select_reads_size(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                               const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, size_t *out_len)
{
    return select_run(c, (const u8 *)d_naf, naf_len, o, segs, strand, n_segs, nullptr, 0, out_len, true, true, 1, select_emit);
}
extern "C" int naf_gpu_unnaf_select_reads(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_unnaf_opts *o,
                                          const naf_gpu_segment *segs, const uint8_t *strand, size_t n_segs, void *d_out, size_t out_cap, size_t *out_len)
{
    int rc = select_run(c, (const u8 *)d_naf, naf_len, o, segs, strand, n_segs, (u8 *)d_out, out_cap, out_len, false, true, 1, select_emit);
    if (c) arena_settle(c);
    return rc;
}
