// locate.h -- IUPAC motifs on either strand, searched in the packed 4-bit stream (naf_gpu_compile_motif, naf_gpu_unnaf_locate_count,
// naf_gpu_unnaf_locate).  Part of emit.hip (included by it, behind emit_select.h): the front of the call, the pieces and the decode of
// a piece's bytes are payload.h's (records_front, piece_plan, PieceSweep); this file holds the motif compiler, the two kernels and their
// launches; the byte-wise load in front of the stream's end is packed.h's (packed_tail), the letter table payload.h's (base_code).
//
// In the code table "-TGKCYSBAWRDMHVN" a base is a SET of nucleotides (A = 8, C = 4, G = 2, T/U = 1, N = 15, '-' = 0), so
//   a stored base c matches a pattern letter p   <=>   c != 0 && (c & ~p) == 0
// and the complement of a code is the code with its four bits reversed.  The contract (include/naf_gpu.h carries it too):
//   patterns   1 .. 32 letters of ACGTU RYSWKM BDHV N in either case, U = T in DNA and RNA archives alike; '-', the empty string and
//              anything else are rejected.
//   matching   letter j against stored base g + j.  A stored ambiguous base matches only letters that contain all of it (stored N:
//              pattern N only; a gap: nothing).  The soft mask plays no part and is not decoded.  A hit lies inside ONE record; bases
//              behind the last record of a malformed archive and the padding nibble of an odd stream are never matched.  Every start
//              position is a hit, overlapping ones too.
//   strands    mask 1 = as stored, 2 = reverse, 3 = both.  A reverse hit at [begin, begin + m) says that the reverse complement of
//              those stored bases matches the pattern -- the stored bases match the pattern reversed with every code bit-reversed.
//              Coordinates are the forward ones.  A pattern that is its own reverse complement gives two hits a place on both strands.
//   order      ascending (record, begin), then pattern number, then strand (0 before 1); the same on every run.
//
// A window of 32 bases is 128 bits, base j in bits 4j .. 4j + 3 (the stream's own order: the first base of a byte is its low nibble).
// One combination of pattern and strand is four 64-bit masks: ~p in the nibbles of its letters (0 behind them) and a 1 in the lowest
// bit of each of those nibbles; against a window W and the "this nibble is zero" flags Z of W (made once per window)
//   hit  <=>  ((W & ~p) | (Z & ones)) == 0
// Two passes over the packed bytes, a wavefront per tile of 4096 bases, 64 positions a lane: a lane loads its 32 bytes and the 16
// behind them and moves the window on by a 128-bit funnel shift of one nibble a step.  k_locate<false> counts -- per tile, per lane
// and per combination (a ballot per test, summed in the lane that owns the combination; one atomic a tile and combination at the
// end) --, the tile counts are scanned, and k_locate<true> recomputes the hits of the tiles that have any and stores them at the place
// a wave prefix sum over the lanes' counts gives.  Tiles start at the searched range's first base rounded down to an even one, so a
// lane's bases always start on a byte.
#pragma once

#define LOC_TILE 4096u
#define LOC_MAX_PATTERNS 16
#define LOC_MAX_COMBOS 32
#define LOC_PIECE_DEFAULT (1ull << 31)       // bases searched per decode of a whole-archive search (NAF_GPU_LOCATE_PIECE)

struct LocCombo { u64 nl, nh, ol, oh; };     // ~p of letters 0..15 / 16..31 (0 behind the pattern); 1 in bit 0 of every nibble that holds a letter
struct LocPats { LocCombo c[LOC_MAX_COMBOS]; u32 len[LOC_MAX_COMBOS]; u8 pat[LOC_MAX_COMBOS], strand[LOC_MAX_COMBOS]; u32 n; };

// bit 4j set where nibble j of w is zero
__device__ __forceinline__ u64 zero_nibbles(u64 w) { u64 t = w | (w >> 1); t |= t >> 2; return ~t & 0x1111111111111111ull; }

// WRITE = false: tile_cnt[t] = hits of tile t, lane_cnt[64 t + lane] = hits of a lane (written for tiles that have hits),
//                combo_cnt[k] += hits of combination k.
// WRITE = true:  the hits of tile t at hits[out_base + tile_off[t] ...], in position order; a tile without hits returns at once.
// LONG: a pattern is longer than 16 letters (the upper half of the window takes part).
// seq: pointer to packed byte 0 of the stream; bytes [.., b_end) of it may be read (the lanes at the range's end load byte by byte).
// Records [r_lo, r_hi) are searched: rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.
template <bool WRITE, bool LONG>
__global__ __launch_bounds__(64) void k_locate(LocPats Q, const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0,
                                               u64 *tile_cnt, u32 *lane_cnt, unsigned long long *combo_cnt,
                                               const u64 *tile_off, u64 out_base, u8 *hits, u64 hit_cap)
{
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    u64 at = 0;
    if (WRITE) {
        const u64 o0 = tile_off[t], o1 = tile_off[t + 1];
        if (o0 == o1) return;
        at = out_base + o0 + wave_prefix_u32(lane_cnt[t * 64 + lane], lane);
    }
    const u64 g = t0 + t * LOC_TILE + lane * 64;                                  // the lane's first position
    const bool active = g < p_hi && g + 64 > p_lo;
    u64 w[6] = { 0, 0, 0, 0, 0, 0 };
    u64 r = 0, rbase = 0, rend = 0;
    if (active) {
        const u64 b0 = g >> 1;
        const u32 nb = LONG ? 48u : 40u;
        if (b0 + nb <= b_end) {
#pragma unroll
            for (u32 k = 0; k < nb / 8; k++) w[k] = ld64(seq + b0 + 8 * k);
        } else packed_tail<(LONG ? 6 : 5)>(seq, b_end, b0, w);
        const u64 x0 = g > p_lo ? g : p_lo;
        r = upper_bound_u64(rec_base, r_lo, r_hi + 1, x0) - 1;                    // rec_base[r_lo] <= x0 < rec_base[r_hi]: r_lo <= r < r_hi
        rbase = rec_base[r]; rend = rec_base[r + 1];
    }
    u32 own = 0, mine = 0;
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        u64 lo = w[k], hi = w[k + 1], nx = LONG ? w[k + 2] : 0;
#pragma unroll 1
        for (u32 j = 0; j < 16; j++) {
            const u64 x = g + 16 * k + j;
            const bool in = active && x >= p_lo && x < p_hi;
            if (in) while (x >= rend && r + 1 < r_hi) { r++; rbase = rend; rend = rec_base[r + 1]; }   // (empty records share a base: the last of them holds x)
            const u32 room = !in || x >= rend ? 0u : (rend - x < 32 ? (u32)(rend - x) : 32u);
            const u64 zl = zero_nibbles(lo), zh = LONG ? zero_nibbles(hi) : 0;
            for (u32 q = 0; q < Q.n; q++) {
                u64 miss = (lo & Q.c[q].nl) | (zl & Q.c[q].ol);
                if (LONG) miss |= (hi & Q.c[q].nh) | (zh & Q.c[q].oh);
                const bool hit = miss == 0 && Q.len[q] <= room;
                if (!WRITE) {
                    const u32 n = (u32)__popcll(__ballot(hit));
                    if (lane == q) mine += n;
                    own += hit;
                } else if (hit) {
                    if (at < hit_cap) { u8 *o = hits + at * 24; st64(o, r); st64(o + 8, x - rbase); st32(o + 16, Q.pat[q]); st32(o + 20, Q.strand[q]); }
                    at++;
                }
            }
            lo = (lo >> 4) | (hi << 60);
            if (LONG) { hi = (hi >> 4) | (nx << 60); nx >>= 4; } else hi >>= 4;
        }
    }
    if (!WRITE) {
        const u32 tot = wave_sum_u32(own);
        if (lane == 0) tile_cnt[t] = tot;
        if (tot) lane_cnt[t * 64 + lane] = own;
        if (lane < Q.n && mine) atomicAdd(&combo_cnt[lane], (unsigned long long)mine);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// letter -> 4-bit set; 0 = no pattern letter (a gap is none)
static u8 motif_code(char ch) { const int k = base_code(ch); return k > 0 ? (u8)k : 0; }
// 0, or 1 + the index of the letter that is none; -1: the length is not 1 .. 32
static int motif_compile(const char *text, u8 fwd[32], u8 rev[32], size_t *len)
{
    const size_t m = strlen(text);
    if (m < 1 || m > 32) return -1;
    for (size_t j = 0; j < m; j++) { fwd[j] = motif_code(text[j]); if (!fwd[j]) return 1 + (int)j; }
    for (size_t j = 0; j < m; j++) { const u8 p = fwd[m - 1 - j]; rev[j] = (u8)(((p & 1) << 3) | ((p & 2) << 1) | ((p & 4) >> 1) | (p >> 3)); }
    for (size_t j = m; j < 32; j++) fwd[j] = rev[j] = 0;
    *len = m;
    return 0;
}
extern "C" int naf_gpu_compile_motif(const char *text, uint8_t fwd[32], uint8_t rev[32], size_t *len)
{
    if (!text || !fwd || !rev || !len) return NAF_GPU_EARG;
    return motif_compile(text, fwd, rev, len) ? NAF_GPU_EARG : 0;
}
static LocCombo motif_masks(const u8 code[32], size_t m)
{
    LocCombo q = { 0, 0, 0, 0 };
    for (size_t j = 0; j < m; j++) {
        const u64 np = (u64)(~code[j] & 15) << (4 * (j & 15)), one = 1ull << (4 * (j & 15));
        if (j < 16) { q.nl |= np; q.ol |= one; } else { q.nh |= np; q.oh |= one; }
    }
    return q;
}

// ---- what the exact search and the one with mismatches (locate_near.h) share on the host; who: the caller's name in the messages ----
// The checks of the arguments and the walk over the blob of patterns: each(k, text) takes pattern k and returns 0 or the error it set.
template <typename Each>
static int motif_walk(naf_gpu_ctx *c, const char *who, const char *h_patterns, size_t patterns_bytes, size_t n_patterns, int strands, Each each)
{
    if (n_patterns < 1 || n_patterns > LOC_MAX_PATTERNS) return ctx_fail(c, NAF_GPU_EARG, "%s: %zu patterns given, 1 to %d can be searched in one call", who, n_patterns, LOC_MAX_PATTERNS);
    if (strands < 1 || strands > 3) return ctx_fail(c, NAF_GPU_EARG, "%s: strand mask %d is none of 1 (as stored), 2 (reverse), 3 (both)", who, strands);
    if (!h_patterns) return ctx_fail(c, NAF_GPU_EARG, "%s: no patterns given (h_patterns is NULL)", who);
    size_t at = 0;
    for (size_t k = 0; k < n_patterns; k++) {
        const void *z = at < patterns_bytes ? memchr(h_patterns + at, 0, patterns_bytes - at) : nullptr;
        if (!z) return ctx_fail(c, NAF_GPU_EARG, "%s: %zu patterns announced, %zu zero-terminated strings in %zu bytes", who, n_patterns, k, patterns_bytes);
        const int rc = each(k, h_patterns + at); if (rc) return rc;
        at = (size_t)((const char *)z - h_patterns) + 1;
    }
    return 0;
}
static int motif_length_fail(naf_gpu_ctx *c, const char *who, size_t k, size_t letters)
{
    return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu has %zu letters, a pattern has 1 to 32", who, k, letters);
}
// pos: the 1-based position in the text of the letter that is none
static int motif_letter_fail(naf_gpu_ctx *c, const char *who, size_t k, const char *text, int pos)
{
    const unsigned char ch = (unsigned char)text[pos - 1];
    if (ch >= 33 && ch < 127) return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu: letter '%c' (position %d) is no IUPAC nucleotide code", who, k, ch, pos);
    return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu: letter '\\x%02X' (position %d) is no IUPAC nucleotide code", who, k, ch, pos);
}
// The front of the call and its pieces; count comes back 0 when there is nothing to search.
static int locate_front(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const char *who, u64 first, u64 *count, UnnafPlan &pl, std::vector<RecPiece> &pieces)
{
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, who, "nucleotide motifs cannot be searched", first, count, pl);
    if (rc || !*count) return rc;
    return piece_plan(c, pl.P, first, *count, "LOCATE_PIECE", LOC_PIECE_DEFAULT, pieces);
}
// The two passes over the pieces.  launch(writing, pc, tl, tile_cnt, lane_cnt, before) launches the caller's kernel: the counting one
// (tile_cnt, lane_cnt and the caller's sums) or the one that writes (tile_cnt scanned: the tiles' offsets; before: the hits of the pieces
// in front).  d_sums: the caller's device counters, zeroed before every sweep.  Too small a capacity is found before anything is written.
template <typename Launch>
static int locate_sweeps(PieceSweep &sw, const std::vector<RecPiece> &pieces, bool write, const void *d_hits, size_t hit_cap, void *d_sums, size_t sums_bytes, u64 *n_hits, Launch launch)
{
    naf_gpu_ctx *c = sw.c;
    return count_then_write(sw, pieces, LOC_TILE, { "hits", write, hit_cap, d_sums, sums_bytes }, n_hits,
                            [&](const RecPiece &pc, const PieceSweep::Tiles &tl, bool writing, u64 before, u64 *here) -> int {
        const u64 ntiles = tl.ntiles;
        u64 *tile_cnt = arena_new<u64>(c, ntiles + 2); u32 *lane_cnt = arena_new<u32>(c, ntiles * 64);
        if (!tile_cnt || !lane_cnt) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(tile_cnt + ntiles, 0, 8, c->stream));
        launch(false, pc, tl, tile_cnt, lane_cnt, before);
        int r = tile_totals(c, ntiles, tile_cnt, here); if (r) return r;
        if (writing && *here) {
            if (before + *here > hit_cap) return NAF_GPU_ECAP;
            if (!d_hits) return NAF_GPU_EARG;
            launch(true, pc, tl, tile_cnt, lane_cnt, before);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return 0;
    });
}

// per_pattern: n_patterns x 2 counts (host), or nullptr.  write: the hits go to d_hits (hit_cap entries); too small a capacity is found
// before anything is written.
static int locate_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns, int strands,
                      u64 first, u64 count, u8 *d_hits, size_t hit_cap, u64 *n_hits, u64 *per_pattern, bool write)
{
    if (!c || !d_naf || !n_hits) return NAF_GPU_EARG;
    *n_hits = 0;
    LocPats Q; memset(&Q, 0, sizeof Q);
    bool any_long = false;
    int rc = motif_walk(c, "locate", h_patterns, patterns_bytes, n_patterns, strands, [&](size_t k, const char *text) -> int {
        u8 fwd[32], rev[32]; size_t m = 0;
        const int bad = motif_compile(text, fwd, rev, &m);
        if (bad < 0) return motif_length_fail(c, "locate", k, strlen(text));
        if (bad > 0) return motif_letter_fail(c, "locate", k, text, bad);
        for (int s = 0; s < 2; s++) if (strands & (1 << s)) {
            Q.c[Q.n] = motif_masks(s ? rev : fwd, m); Q.len[Q.n] = (u32)m; Q.pat[Q.n] = (u8)k; Q.strand[Q.n] = (u8)s; Q.n++;
        }
        any_long = any_long || m > 16;
        return 0;
    });
    if (rc) return rc;
    if (per_pattern) for (size_t k = 0; k < 2 * n_patterns; k++) per_pattern[k] = 0;
    UnnafPlan pl; std::vector<RecPiece> pieces;
    rc = locate_front(c, d_naf, naf_len, "locate", first, &count, pl, pieces);
    if (rc || !count) return rc;
    const EmitP &P = pl.P;

    u64 *combo_cnt = arena_new<u64>(c, LOC_MAX_COMBOS); if (!combo_cnt) return NAF_GPU_ENOMEM;
    PieceSweep sw(c, d_naf, pl, "locate");
    rc = locate_sweeps(sw, pieces, write, d_hits, hit_cap, combo_cnt, LOC_MAX_COMBOS * 8, n_hits,
                       [&](bool writing, const RecPiece &pc, const PieceSweep::Tiles &tl, u64 *tile_cnt, u32 *lane_cnt, u64 before) {
#define LOC_LAUNCH(W, L, name) LAUNCH(c, name, (k_locate<W, L>), (u32)tl.ntiles, 64, 0, Q, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, tile_cnt, lane_cnt, (unsigned long long *)combo_cnt, (const u64 *)tile_cnt, before, d_hits, (u64)hit_cap)
        if (writing) { if (any_long) LOC_LAUNCH(true, true, "unnaf_locate_write"); else LOC_LAUNCH(true, false, "unnaf_locate_write"); }
        else { if (any_long) LOC_LAUNCH(false, true, "unnaf_locate_count"); else LOC_LAUNCH(false, false, "unnaf_locate_count"); }
#undef LOC_LAUNCH
    });
    if (rc) return rc;
    if (per_pattern) {
        u64 cc[LOC_MAX_COMBOS];
        if ((rc = ctx_readback(c, cc, combo_cnt, sizeof cc))) return rc;
        for (u32 q = 0; q < Q.n; q++) per_pattern[2 * Q.pat[q] + Q.strand[q]] = cc[q];
    }
    if (ctx_tracing(c)) ctx_trace(c, "[locate] patterns %zu records %llu..%llu pieces %zu sequence bytes decoded %llu of %llu hits %llu\n", n_patterns,
                                  (unsigned long long)first, (unsigned long long)(first + count), pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes, (unsigned long long)*n_hits);
    return 0;
}

extern "C" int naf_gpu_unnaf_locate_count(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns, int strands,
                                          uint64_t first, uint64_t count, uint64_t *n_hits, uint64_t *per_pattern)
{
    int rc = locate_run(c, (const u8 *)d_naf, naf_len, h_patterns, patterns_bytes, n_patterns, strands, first, count, nullptr, 0, n_hits, per_pattern, false);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_locate(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns, int strands,
                                    uint64_t first, uint64_t count, naf_gpu_hit *d_hits, size_t hit_cap, uint64_t *n_hits)
{
    int rc = locate_run(c, (const u8 *)d_naf, naf_len, h_patterns, patterns_bytes, n_patterns, strands, first, count, (u8 *)d_hits, hit_cap, n_hits, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
