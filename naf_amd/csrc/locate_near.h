// locate_near.h -- IUPAC motifs with a budget of mismatches and letters that must match, searched in the packed 4-bit stream
// (naf_gpu_compile_motif_near, naf_gpu_unnaf_locate_near_count, naf_gpu_unnaf_locate_near).  Part of emit.hip (included by it, behind
// locate.h): the window, its masks and the rule "c matches p  <=>  c != 0 && (c & ~p) == 0" are locate.h's, the front of the call, the
// pieces and the sweeps payload.h's (records_front, piece_plan, PieceSweep, count_then_write, tile_totals) through locate.h's host
// front (motif_walk, locate_front, locate_sweeps), which both searches share.  This file holds the bracket parser, the kernel and its
// launches.  The contract (include/naf_gpu.h carries it too):
//   patterns   those of locate.h; a run of letters in square brackets must match: GAGTCCGAGCAGAAGAAGAA[NGG].  Brackets do not nest and
//              are not empty; 1 .. 32 letters, the brackets not counted.
//   hit        a start position where the pattern's letters lie inside ONE record, no bracketed letter mismatches and at most
//              budget[k] of the others do (0 .. 8; above 0 it is smaller than the number of unbracketed letters).  A stored gap
//              mismatches every letter, a stored N every letter but N.  Every start position counts.
//   strands    as in locate.h: a reverse hit at [begin, begin + m) says that the reverse complement of those stored bases is within
//              the budget; `where` is told by the pattern's letters as written: on the reverse strand letter j faces base begin + m - 1 - j.
//   order      ascending (record, begin), then pattern number, then strand; the same on every run and for every piece size.
//
// The bit work.  locate.h's word  miss = (W & ~p) | (Z & ones)  is non-zero exactly in the nibbles of the letters that mismatch.
// Collapsed to bit 0 of every nibble (t = miss | miss >> 1; t |= t >> 2; t &= 0x1111..) it is one bit a letter:
//   hit  <=>  (t & fixed) == 0  &&  popcount(t) <= budget  &&  len <= room
// and the popcount IS the number of mismatches among the unbracketed letters, since a hit has none among the others.  Only the write
// pass, and only for a hit, packs t's bits to 16 + 16 adjacent ones (loc_pack16) -- bit i = window base i mismatches -- and turns
// them round for a reverse combination (__brev(x) >> (32 - m)), so that bit j is letter j of the pattern as written.
// The kernel has k_locate's shape: a wavefront per tile of 4096 bases, 64 positions a lane, the window loaded once and moved on by the
// nibble funnel shift, the record walk and `room` as they are.  The counting pass keeps a histogram [combination][mismatches] of 32 x 9
// cells in LDS -- a hit adds 1 to its cell with an LDS atomic; hits are rare, so the branch is seldom taken -- and the wave adds every
// non-zero cell to the call's counters with one atomic at the end.  (Nine ballots a test, one per distance, was the other scheme:
// DESIGN.md 8k has both.)
#pragma once

#define LOCN_MAX_MISMATCHES 8                // NAF_GPU_LOCATE_MAX_MISMATCHES
#define LOCN_DIST (LOCN_MAX_MISMATCHES + 1)
#define LOCN_CELLS (LOC_MAX_COMBOS * LOCN_DIST)

// LocCombo and, with a 1 in bit 0 of every nibble that holds a bracketed letter, fl / fh
struct LocNearCombo { u64 nl, nh, ol, oh, fl, fh; };
struct LocNearPats { LocNearCombo c[LOC_MAX_COMBOS]; u32 len[LOC_MAX_COMBOS], budget[LOC_MAX_COMBOS]; u8 pat[LOC_MAX_COMBOS], strand[LOC_MAX_COMBOS]; u32 n; };
static_assert(sizeof(LocNearPats) + 16 * 8 <= 4096, "k_locate_near takes its combinations by value: they and its other arguments stay within the 4 KiB of kernel arguments");

// bit 0 of every nibble that is not zero
__device__ __forceinline__ u64 loc_collapse(u64 m) { u64 t = m | (m >> 1); t |= t >> 2; return t & 0x1111111111111111ull; }
// bit 0 of each of a word's sixteen nibbles -> sixteen adjacent bits (runs_pack8's steps, one more)
__device__ __forceinline__ u32 loc_pack16(u64 y)
{
    y = (y | (y >> 3)) & 0x0303030303030303ull; y = (y | (y >> 6)) & 0x000F000F000F000Full; y = (y | (y >> 12)) & 0x000000FF000000FFull;
    return (u32)((y | (y >> 24)) & 0xFFFFu);
}

// WRITE = false: tile_cnt[t] = hits of tile t, lane_cnt[64 t + lane] = hits of a lane (written for tiles that have hits),
//                cell_cnt[9 q + d] += hits of combination q with exactly d mismatches.
// WRITE = true:  the hits of tile t at hits[out_base + tile_off[t] ...], 32 bytes each, in position order; a tile without hits returns at once.
// LONG, seq, b_end, the records and t0: as k_locate's.
template <bool WRITE, bool LONG>
__global__ __launch_bounds__(64) void k_locate_near(LocNearPats Q, const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0,
                                                    u64 *tile_cnt, u32 *lane_cnt, unsigned long long *cell_cnt,
                                                    const u64 *tile_off, u64 out_base, u8 *hits, u64 hit_cap)
{
    __shared__ u32 cells[WRITE ? 1 : LOCN_CELLS];
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    u64 at = 0;
    if (WRITE) {
        const u64 o0 = tile_off[t], o1 = tile_off[t + 1];
        if (o0 == o1) return;
        at = out_base + o0 + wave_prefix_u32(lane_cnt[t * 64 + lane], lane);
    } else {
        for (u32 k = lane; k < LOCN_CELLS; k += 64) cells[k] = 0;
        __syncthreads();
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
    u32 own = 0;
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
                const u64 tl = loc_collapse((lo & Q.c[q].nl) | (zl & Q.c[q].ol));
                const u64 th = LONG ? loc_collapse((hi & Q.c[q].nh) | (zh & Q.c[q].oh)) : 0;
                const u32 d = (u32)__popcll(tl) + (LONG ? (u32)__popcll(th) : 0u);
                bool hit = (tl & Q.c[q].fl) == 0 && d <= Q.budget[q] && Q.len[q] <= room;
                if (LONG) hit = hit && (th & Q.c[q].fh) == 0;
                if (!WRITE) {
                    if (hit) { atomicAdd(&cells[q * LOCN_DIST + d], 1u); own++; }
                } else if (hit) {
                    if (at < hit_cap) {
                        u32 wh = loc_pack16(tl) | (LONG ? loc_pack16(th) << 16 : 0u);
                        if (Q.strand[q]) wh = __brev(wh) >> (32 - Q.len[q]);
                        u8 *o = hits + at * 32;
                        st64(o, r); st64(o + 8, x - rbase); st32(o + 16, Q.pat[q]); st32(o + 20, Q.strand[q]); st32(o + 24, d); st32(o + 28, wh);
                    }
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
        __syncthreads();
        if (tot) {
            lane_cnt[t * 64 + lane] = own;
            for (u32 k = lane; k < Q.n * LOCN_DIST; k += 64) { const u32 v = cells[k]; if (v) atomicAdd(&cell_cnt[k], (unsigned long long)v); }
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// What is wrong with a pattern: *pos is the 1-based position in the text of the character that shows it.
enum { MOTIF_OK = 0, MOTIF_LENGTH, MOTIF_LETTER, MOTIF_NESTED, MOTIF_UNOPENED, MOTIF_EMPTY, MOTIF_UNCLOSED };
// fixed: bit j set when letter j (the brackets not counted) stands in brackets; *len: the letters
static int motif_compile_near(const char *text, u8 fwd[32], u8 rev[32], u32 *fixed, size_t *len, int *pos)
{
    size_t letters = 0;
    for (const char *p = text; *p; p++) letters += *p != '[' && *p != ']';
    *pos = 0;
    if (letters > 32) return MOTIF_LENGTH;
    size_t m = 0, open_at = 0; bool open = false; u32 fx = 0;
    for (size_t i = 0; text[i]; i++) {
        *pos = (int)i + 1;
        if (text[i] == '[') { if (open) return MOTIF_NESTED; open = true; open_at = m; continue; }
        if (text[i] == ']') { if (!open) return MOTIF_UNOPENED; if (m == open_at) return MOTIF_EMPTY; open = false; continue; }
        fwd[m] = motif_code(text[i]); if (!fwd[m]) return MOTIF_LETTER;
        if (open) fx |= 1u << m;
        m++;
    }
    if (open) return MOTIF_UNCLOSED;
    *pos = 0;
    if (m < 1) return MOTIF_LENGTH;
    for (size_t j = 0; j < m; j++) { const u8 p = fwd[m - 1 - j]; rev[j] = (u8)(((p & 1) << 3) | ((p & 2) << 1) | ((p & 4) >> 1) | (p >> 3)); }
    for (size_t j = m; j < 32; j++) fwd[j] = rev[j] = 0;
    *fixed = fx; *len = m;
    return MOTIF_OK;
}
extern "C" int naf_gpu_compile_motif_near(const char *text, uint8_t fwd[32], uint8_t rev[32], uint32_t *fixed, size_t *len)
{
    if (!text || !fwd || !rev || !fixed || !len) return NAF_GPU_EARG;
    u8 f[32], r[32]; int pos;                                                      // (nothing of the caller's is touched by what is no pattern)
    if (motif_compile_near(text, f, r, fixed, len, &pos)) return NAF_GPU_EARG;
    memcpy(fwd, f, 32); memcpy(rev, r, 32);
    return 0;
}
// fixed: by position in the window (for the reverse strand the caller turns the pattern's mask round)
static LocNearCombo motif_masks_near(const u8 code[32], size_t m, u32 fixed)
{
    const LocCombo e = motif_masks(code, m);
    LocNearCombo q = { e.nl, e.nh, e.ol, e.oh, 0, 0 };
    for (size_t j = 0; j < m; j++) if (fixed >> j & 1) { if (j < 16) q.fl |= 1ull << (4 * j); else q.fh |= 1ull << (4 * (j - 16)); }
    return q;
}

// per_pattern: n_patterns x 2 x 9 counts (host), or nullptr.  write: the hits go to d_hits (hit_cap entries); too small a capacity is
// found before anything is written.  The walk over the patterns, the front and the two passes are locate.h's (motif_walk, locate_front,
// locate_sweeps); what is this file's own: the brackets, the budgets, the nine distances and the kernel.
static int locate_near_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns, const u32 *h_budget,
                           int strands, u64 first, u64 count, u8 *d_hits, size_t hit_cap, u64 *n_hits, u64 *per_pattern, bool write)
{
    static const char who[] = "locate-near";
    if (!c || !d_naf || !n_hits) return NAF_GPU_EARG;
    *n_hits = 0;
    LocNearPats Q; memset(&Q, 0, sizeof Q);
    bool any_long = false; u32 top = 0;
    int rc = motif_walk(c, who, h_patterns, patterns_bytes, n_patterns, strands, [&](size_t k, const char *text) -> int {
        if (!h_budget) return ctx_fail(c, NAF_GPU_EARG, "%s: no budgets given (h_max_mismatches is NULL)", who);
        u8 fwd[32], rev[32]; size_t m = 0; u32 fixed = 0; int pos = 0;
        const int bad = motif_compile_near(text, fwd, rev, &fixed, &m, &pos);
        if (bad == MOTIF_LENGTH) {
            size_t letters = 0; for (const char *p = text; *p; p++) letters += *p != '[' && *p != ']';
            return motif_length_fail(c, who, k, letters);
        }
        if (bad == MOTIF_LETTER) return motif_letter_fail(c, who, k, text, pos);
        if (bad) return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu: %s (position %d)", who, k,
                                 bad == MOTIF_NESTED ? "'[' inside brackets: they do not nest" : bad == MOTIF_UNOPENED ? "']' without a '[' in front of it" :
                                 bad == MOTIF_EMPTY ? "empty brackets" : "'[' is never closed", pos);
        const u32 budget = h_budget[k], free_letters = (u32)m - (u32)__builtin_popcount(fixed);
        if (budget > LOCN_MAX_MISMATCHES) return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu: %u mismatches allowed, the most is %d", who, k, budget, LOCN_MAX_MISMATCHES);
        if (budget && budget >= free_letters)
            return ctx_fail(c, NAF_GPU_EARG, "%s: pattern %zu: %u mismatches allowed among %u letters outside brackets: every place would be a hit", who, k, budget, free_letters);
        u32 fixed_rev = 0; for (size_t j = 0; j < m; j++) if (fixed >> j & 1) fixed_rev |= 1u << (m - 1 - j);
        for (int s = 0; s < 2; s++) if (strands & (1 << s)) {
            Q.c[Q.n] = motif_masks_near(s ? rev : fwd, m, s ? fixed_rev : fixed);
            Q.len[Q.n] = (u32)m; Q.pat[Q.n] = (u8)k; Q.strand[Q.n] = (u8)s; Q.budget[Q.n] = budget; Q.n++;
        }
        any_long = any_long || m > 16;
        top = budget > top ? budget : top;
        return 0;
    });
    if (rc) return rc;
    if (per_pattern) for (size_t k = 0; k < 2 * LOCN_DIST * n_patterns; k++) per_pattern[k] = 0;
    UnnafPlan pl; std::vector<RecPiece> pieces;
    rc = locate_front(c, d_naf, naf_len, who, first, &count, pl, pieces);
    if (rc || !count) return rc;
    const EmitP &P = pl.P;

    u64 *cell_cnt = arena_new<u64>(c, LOCN_CELLS); if (!cell_cnt) return NAF_GPU_ENOMEM;
    PieceSweep sw(c, d_naf, pl, who);
    rc = locate_sweeps(sw, pieces, write, d_hits, hit_cap, cell_cnt, LOCN_CELLS * 8, n_hits,
                       [&](bool writing, const RecPiece &pc, const PieceSweep::Tiles &tl, u64 *tile_cnt, u32 *lane_cnt, u64 before) {
#define LOCN_LAUNCH(W, L, name) LAUNCH(c, name, (k_locate_near<W, L>), (u32)tl.ntiles, 64, 0, Q, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, tile_cnt, lane_cnt, (unsigned long long *)cell_cnt, (const u64 *)tile_cnt, before, d_hits, (u64)hit_cap)
        if (writing) { if (any_long) LOCN_LAUNCH(true, true, "unnaf_locate_near_write"); else LOCN_LAUNCH(true, false, "unnaf_locate_near_write"); }
        else { if (any_long) LOCN_LAUNCH(false, true, "unnaf_locate_near_count"); else LOCN_LAUNCH(false, false, "unnaf_locate_near_count"); }
#undef LOCN_LAUNCH
    });
    if (rc) return rc;
    if (per_pattern) {
        u64 cc[LOCN_CELLS];
        if ((rc = ctx_readback(c, cc, cell_cnt, sizeof cc))) return rc;
        for (u32 q = 0; q < Q.n; q++) for (u32 d = 0; d < LOCN_DIST; d++) per_pattern[(2 * Q.pat[q] + Q.strand[q]) * LOCN_DIST + d] = cc[q * LOCN_DIST + d];
    }
    if (ctx_tracing(c)) ctx_trace(c, "[locate-near] patterns %zu budget max %u records %llu..%llu pieces %zu sequence bytes decoded %llu of %llu hits %llu\n", n_patterns, top,
                                  (unsigned long long)first, (unsigned long long)(first + count), pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes, (unsigned long long)*n_hits);
    return 0;
}

extern "C" int naf_gpu_unnaf_locate_near_count(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                                               const uint32_t *h_max_mismatches, int strands, uint64_t first, uint64_t count, uint64_t *n_hits, uint64_t *per_pattern)
{
    int rc = locate_near_run(c, (const u8 *)d_naf, naf_len, h_patterns, patterns_bytes, n_patterns, h_max_mismatches, strands, first, count, nullptr, 0, n_hits, per_pattern, false);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_locate_near(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const char *h_patterns, size_t patterns_bytes, size_t n_patterns,
                                         const uint32_t *h_max_mismatches, int strands, uint64_t first, uint64_t count, naf_gpu_near_hit *d_hits, size_t hit_cap, uint64_t *n_hits)
{
    int rc = locate_near_run(c, (const u8 *)d_naf, naf_len, h_patterns, patterns_bytes, n_patterns, h_max_mismatches, strands, first, count, (u8 *)d_hits, hit_cap, n_hits, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
