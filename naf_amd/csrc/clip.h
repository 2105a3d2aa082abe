// clip.h -- 3' adapters clipped from reads, decided in the packed 4-bit stream (naf_gpu_clip_budgets, naf_gpu_unnaf_clip).  Part of
// emit.hip (included by it, behind trim.h): the window, its masks and the rule "c matches p  <=>  c != 0 && (c & ~p) == 0" are locate.h's,
// the collapse of the mismatch word to one bit a letter locate_near.h's, the front of the call, the pieces and the decode of a piece's
// bytes payload.h's (records_front, piece_plan, PieceSweep), the walk over the blob of adapters locate.h's (motif_walk).  This file holds
// the two kernels and the launches.  The contract is include/naf_gpu.h's.
//
// A start x of record r (window [begin_r, end_r) of it) overlaps adapter k in L = min(m_k, end_r - x) letters; it is a candidate when
// L >= min_overlap and at most budget[k][L] of the adapter's first L letters mismatch.  The clip point is the smallest candidate of the
// record, the lowest adapter number at equal x.
//
// The stage: k_bounds_stage (reads.h) with the flags cut to NAF_GPU_TRIM_ERRORS, the one a clip row carries on.  Its verdict on the bounds
// rows is looked at once, at the end of the call; until then the row copy holds back (k_row_copy's guard).
// k_clip_mark: k_locate_near's skeleton -- a wavefront per tile of 4096 bases, 64 positions a lane, the 32-base window loaded once and
// moved on by the nibble funnel shift, the record walk by rec_base.  What is new: `room` is min(32, end_r - x) of the record's WINDOW, the
// collapsed mismatch word is cut to its lowest `room` letters before the popcount, the budget is looked up by the overlap (for a full
// overlap in the kernel's arguments, else in a 16 x 33 byte table in LDS), and a lane takes only its first candidate per record: every
// later one of the record is larger.  A step at which no lane of the wave is within 32 bases of its window's end (16 when no adapter is
// longer) cuts nothing and reads no table: the loop of locate_near.h with a budget per adapter; the walk compares 32-bit offsets from the
// lane's first base.  The candidates of one record are combined by a 64-bit atomicMin on a key per record of the piece,
// preset to all ones:  key = x << 16 | adapter << 8 | mismatches.  A minimum does not depend on the order, so the table is the same on
// every run; at most one atomic a lane and record with a candidate.
// k_clip_finish: a lane per record of the piece turns key and window into the row (5 u64, in the arena) and adds the totals (wg_sums)
// and the [adapter][overlap] histogram: lanes, then the workgroup in LDS, then one atomic per non-zero cell and workgroup.
#pragma once

#define CLIP_TILE 4096u
#define CLIP_MAX_ADAPTERS 16                  // NAF_GPU_CLIP_MAX_ADAPTERS
#define CLIP_ROW_U64 5u
#define CLIP_PIECE_DEFAULT (1ull << 31)       // bases swept per decode (NAF_GPU_CLIP_PIECE)
#define CLIP_TOTALS 8u                        // reads, clipped, kept, bases, kept_bases, removed_bases, n_short, n_errors
#define CLIP_CELLS (CLIP_MAX_ADAPTERS * 33)
#define CLIP_NO_KEY 0xFFFFFFFFFFFFFFFFull

// full[q]: budget[q][len[q]], or CLIP_NEVER when len[q] < min_overlap (no overlap of that adapter is long enough: no count of mismatches is below it)
#define CLIP_NEVER (-1)
struct ClipPats { LocCombo c[CLIP_MAX_ADAPTERS]; u32 len[CLIP_MAX_ADAPTERS]; int full[CLIP_MAX_ADAPTERS]; u8 budget[CLIP_CELLS]; u32 n, min_overlap; };
static_assert(sizeof(ClipPats) + 16 * 8 <= 4096, "k_clip_mark takes its adapters by value: they and its other arguments stay within the 4 KiB of kernel arguments");

// LONG: an adapter is longer than 16 letters (the upper half of the window takes part).
// seq: pointer to packed byte 0 of the stream; bytes [.., b_end) of it may be read (the lanes at the range's end load byte by byte).
// Records [r_lo, r_hi) are searched: rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.
// win: the staged windows, win[0] that of record r_lo.  keys: one per record, keys[0] that of record r_lo, preset to CLIP_NO_KEY.
template <bool LONG>
__global__ __launch_bounds__(64) void k_clip_mark(ClipPats Q, const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0,
                                                  const u64 *win, unsigned long long *keys)
{
    __shared__ u8 bud[CLIP_CELLS];
    const u32 lane = threadIdx.x;
    for (u32 k = lane; k < CLIP_CELLS; k += 64) bud[k] = Q.budget[k];
    __syncthreads();
    const u64 t = xcd_block();
    const u64 g = t0 + t * CLIP_TILE + lane * 64;                                 // the lane's first position
    const bool active = g < p_hi && g + 64 > p_lo;
    if (!active) return;
    u64 w[6] = { 0, 0, 0, 0, 0, 0 };
    {
        const u64 b0 = g >> 1;
        const u32 nb = LONG ? 48u : 40u;
        if (b0 + nb <= b_end) {
#pragma unroll
            for (u32 k = 0; k < nb / 8; k++) w[k] = ld64(seq + b0 + 8 * k);
        } else packed_tail<(LONG ? 6 : 5)>(seq, b_end, b0, w);
    }
    const u64 x0 = g > p_lo ? g : p_lo;
    u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, x0) - 1;                    // rec_base[r_lo] <= x0 < rec_base[r_hi]: r_lo <= r < r_hi
    u64 rbase = rec_base[r], rend = rec_base[r + 1];
    // Inside the walk everything is an offset from g in 32 bits: a position in front of g is 0, one far behind it CLIP_FAR (the lane looks at
    // its 64 positions and the 32 behind them, no further).
#define CLIP_FAR 4096u
#define CLIP_REL(v) ((v) <= g ? 0u : (v) - g > CLIP_FAR ? CLIP_FAR : (u32)((v) - g))
    const u32 i_lo = CLIP_REL(p_lo), i_hi = CLIP_REL(p_hi);                        // the lane's positions [i_lo, i_hi) are searched
    u32 rend_i = CLIP_REL(rend), wb_i = CLIP_REL(rbase + win[2 * (r - r_lo)]), we_i = CLIP_REL(rbase + win[2 * (r - r_lo) + 1]);   // the record's end and its window
    bool found = false;                                                           // the lane has its candidate of record r
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        u64 lo = w[k], hi = w[k + 1], nx = LONG ? w[k + 2] : 0;
#pragma unroll 1
        for (u32 j = 0; j < 16; j++) {
            const u32 i = 16 * k + j;
            bool cand = false; u32 room = 0;                                      // a start inside its record's window, with `room` bases to the window's end (32: or more)
            if (i >= i_lo && i < i_hi) {
                while (i >= rend_i && r + 1 < r_hi) {                             // (empty records share a base: the last of them holds the position)
                    r++; rbase = rend; rend = rec_base[r + 1];
                    rend_i = CLIP_REL(rend); wb_i = CLIP_REL(rbase + win[2 * (r - r_lo)]); we_i = CLIP_REL(rbase + win[2 * (r - r_lo) + 1]); found = false;
                }
                cand = !found && i >= wb_i && i < we_i;
                room = !cand ? 0u : we_i - i < 32 ? we_i - i : 32u;
            }
            const u64 zl = zero_nibbles(lo), zh = LONG ? zero_nibbles(hi) : 0;
            u32 hit = CLIP_MAX_ADAPTERS, hd = 0;
            // One loop for the whole wave (every lane that has not left is here).  No lane near its window's end -- all of long reads but their
            // last bases --: every adapter overlaps in all its letters, nothing is cut and the budgets are the arguments'.  Else the window is
            // cut to `room` letters in every lane; both loops side by side in one wave cost more than the second alone.
            if (__ballot(cand && room < (LONG ? 32u : 16u)) == 0) {
                if (cand) for (u32 q = 0; q < Q.n; q++) {
                    const u64 tl = loc_collapse((lo & Q.c[q].nl) | (zl & Q.c[q].ol));
                    const u64 th = LONG ? loc_collapse((hi & Q.c[q].nh) | (zh & Q.c[q].oh)) : 0;
                    const u32 d = (u32)__popcll(tl) + (LONG ? (u32)__popcll(th) : 0u);
                    if ((int)d <= Q.full[q]) { hit = q; hd = d; break; }           // the lowest adapter number at this start
                }
            } else if (room >= Q.min_overlap) {
                // the lowest `room` letters of the window: those in front of the window's end
                const u64 ml = room >= 16 ? ~0ull : (1ull << (4 * room)) - 1;
                const u64 mh = room >= 32 ? ~0ull : room <= 16 ? 0ull : (1ull << (4 * (room - 16))) - 1;
                for (u32 q = 0; q < Q.n; q++) {
                    const int allowed = room >= Q.len[q] ? Q.full[q] : (int)bud[q * 33 + room];     // (room < len: the overlap is `room` >= min_overlap)
                    const u64 tl = loc_collapse((lo & Q.c[q].nl) | (zl & Q.c[q].ol)) & ml;
                    const u64 th = LONG ? loc_collapse((hi & Q.c[q].nh) | (zh & Q.c[q].oh)) & mh : 0;
                    const u32 d = (u32)__popcll(tl) + (LONG ? (u32)__popcll(th) : 0u);
                    if ((int)d <= allowed) { hit = q; hd = d; break; }
                }
            }
            if (hit < CLIP_MAX_ADAPTERS) {
                atomicMin(&keys[r - r_lo], (unsigned long long)((g + i - rbase) << 16 | (u64)hit << 8 | hd));
                found = true;
            }
            lo = (lo >> 4) | (hi << 60);
            if (LONG) { hi = (hi >> 4) | (nx << 60); nx >>= 4; } else hi >>= 4;
        }
    }
#undef CLIP_REL
#undef CLIP_FAR
}

struct ClipFinP {
    const u64 *rec_base, *win; const u32 *wflags; const unsigned long long *keys;      // win, wflags, keys: [0] is record r_lo's
    u64 r_lo, r_hi, min_len;
    u32 len[CLIP_MAX_ADAPTERS];
    u64 *rows;                                 // row of record r_lo (5 u64 a row, 8-byte aligned), null: not wanted
    unsigned long long *total, *cells;         // CLIP_TOTALS counters, CLIP_CELLS cells [adapter][overlap]
};

__global__ __launch_bounds__(256) void k_clip_finish(ClipFinP P)
{
    __shared__ unsigned long long tsum[CLIP_TOTALS];
    __shared__ u32 hist[CLIP_CELLS];
    const u32 tid = threadIdx.x;
    if (tid < CLIP_TOTALS) tsum[tid] = 0;
    for (u32 k = tid; k < CLIP_CELLS; k += 256) hist[k] = 0;
    __syncthreads();
    u64 T[CLIP_TOTALS]; for (u32 k = 0; k < CLIP_TOTALS; k++) T[k] = 0;
    const u64 r = P.r_lo + (u64)blockIdx.x * 256 + tid;
    if (r < P.r_hi) {
        const u64 k = r - P.r_lo;
        const u64 begin = P.win[2 * k], wend = P.win[2 * k + 1], key = P.keys[k];
        u64 end = wend; u32 adapter = NAF_GPU_CLIP_NO_ADAPTER, mism = 0, overlap = 0;
        const bool clipped = key != CLIP_NO_KEY;
        if (clipped) {
            end = key >> 16; adapter = (u32)(key >> 8) & 0xFFu; mism = (u32)key & 0xFFu;
            overlap = wend - end < P.len[adapter & 15u] ? (u32)(wend - end) : P.len[adapter & 15u];
            atomicAdd(&hist[(adapter & 15u) * 33 + overlap], 1u);
        }
        const bool is_short = end - begin < P.min_len, errors = P.wflags[k] != 0;
        const u32 flags = (is_short || errors ? (is_short ? NAF_GPU_TRIM_SHORT : 0u) | (errors ? NAF_GPU_TRIM_ERRORS : 0u) : NAF_GPU_TRIM_KEPT) | (clipped ? NAF_GPU_CLIP_CLIPPED : 0u);
        if (P.rows) { u64 *o = P.rows + k * CLIP_ROW_U64; o[0] = r; o[1] = begin; o[2] = end; o[3] = (u64)adapter | (u64)mism << 32; o[4] = (u64)overlap | (u64)flags << 32; }
        T[0] = 1; T[1] = clipped; T[3] = wend - begin; T[5] = wend - end; T[6] = is_short; T[7] = errors;
        if (flags & NAF_GPU_TRIM_KEPT) { T[2] = 1; T[4] = end - begin; }
    }
    wg_sums(T, tsum, P.total);                                                    // (its barrier stands behind the histogram's atomics too)
    for (u32 k = tid; k < CLIP_CELLS; k += 256) if (hist[k]) atomicAdd(&P.cells[k], (unsigned long long)hist[k]);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_clip_budgets(uint64_t num, uint64_t den, unsigned m, uint8_t out[33])
{
    if (!out || den == 0 || m < 1 || m > 32) return NAF_GPU_EARG;
    out[0] = 0;
    for (unsigned L = 1; L <= 32; L++) {
        const unsigned __int128 v = (unsigned __int128)L * num / den;
        out[L] = L > m ? 0 : v > L - 1 ? (uint8_t)(L - 1) : (uint8_t)v;
    }
    return 0;
}

extern "C" int naf_gpu_unnaf_clip(naf_gpu_ctx *c, const void *d_naf_, size_t naf_len, const char *h_adapters, size_t adapters_bytes, size_t n_adapters,
                                  const uint8_t *h_budget, const naf_gpu_clip_opts *o, uint64_t first, uint64_t count, const naf_gpu_trim_row *d_bounds_,
                                  naf_gpu_clip_row *d_rows_, size_t row_cap, uint64_t *n_records, naf_gpu_clip_total *h_total, uint64_t *per_adapter)
{
    static const char who[] = "clip";
    const u8 *d_naf = (const u8 *)d_naf_, *d_bounds = (const u8 *)d_bounds_; u8 *d_rows = (u8 *)d_rows_;
    if (!c || !d_naf || !o || !n_records) return NAF_GPU_EARG;
    *n_records = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    if (n_adapters < 1 || n_adapters > CLIP_MAX_ADAPTERS) return ctx_fail(c, NAF_GPU_EARG, "%s: %zu adapters given, 1 to %d can be clipped in one call", who, n_adapters, CLIP_MAX_ADAPTERS);
    if (per_adapter) for (size_t k = 0; k < 33 * n_adapters; k++) per_adapter[k] = 0;
    if (o->min_overlap < 1 || o->min_overlap > 32) return ctx_fail(c, NAF_GPU_EARG, "%s: min_overlap %u (1 to 32 letters of an adapter)", who, o->min_overlap);
    if (o->min_len == 0) return ctx_fail(c, NAF_GPU_EARG, "%s: min_len 0 (a kept read has at least one base)", who);
    if (!h_budget) return ctx_fail(c, NAF_GPU_EARG, "%s: no budgets given (h_budget is NULL)", who);
    ClipPats Q; memset(&Q, 0, sizeof Q);
    Q.min_overlap = o->min_overlap;
    bool any_long = false;
    int rc = motif_walk(c, who, h_adapters, adapters_bytes, n_adapters, 1, [&](size_t k, const char *text) -> int {
        u8 fwd[32], rev[32]; size_t m = 0;
        const int bad = motif_compile(text, fwd, rev, &m);
        if (bad < 0) {
            const size_t n = strlen(text);
            if (n > 32) return ctx_fail(c, NAF_GPU_EARG, "%s: adapter %zu has %zu letters, an adapter has 1 to 32 (of a 3' adapter the first 32 letters decide the same clip points: give those)", who, k, n);
            return ctx_fail(c, NAF_GPU_EARG, "%s: adapter %zu has no letters, an adapter has 1 to 32", who, k);
        }
        if (bad > 0) {
            const unsigned char ch = (unsigned char)text[bad - 1];
            if (ch >= 33 && ch < 127) return ctx_fail(c, NAF_GPU_EARG, "%s: adapter %zu: letter '%c' (position %d) is no IUPAC nucleotide code", who, k, ch, bad);
            return ctx_fail(c, NAF_GPU_EARG, "%s: adapter %zu: letter '\\x%02X' (position %d) is no IUPAC nucleotide code", who, k, ch, bad);
        }
        const u8 *b = h_budget + 33 * k;
        for (u32 L = o->min_overlap; L <= m; L++) if (b[L] >= L)
            return ctx_fail(c, NAF_GPU_EARG, "%s: adapter %zu: %u mismatches allowed in an overlap of %u letters: every place would be a hit", who, k, (unsigned)b[L], L);
        Q.c[k] = motif_masks(fwd, m); Q.len[k] = (u32)m; Q.full[k] = m >= o->min_overlap ? (int)b[m] : CLIP_NEVER;
        memcpy(Q.budget + 33 * k, b, 33);
        any_long = any_long || m > 16;
        return 0;
    });
    if (rc) return rc;
    Q.n = (u32)n_adapters;
    UnnafPlan pl;
    rc = records_front(c, d_naf, naf_len, FRONT_4BIT, who, "adapters cannot be clipped", first, &count, pl);
    if (rc) { arena_settle(c); return rc; }
    *n_records = count;
    if (!count) { arena_settle(c); return 0; }
    auto run = [&]() -> int {
        const EmitP &P = pl.P;
        if (d_rows && count > row_cap) return cap_fail(c, who, "rows", count, row_cap);
        LAUNCH_LIMIT(c, count, CLIP_ROW_U64, "%s: %llu records are too many for one launch", who, (unsigned long long)count);
        std::vector<RecPiece> pieces;
        if ((rc = piece_plan(c, P, first, count, "CLIP_PIECE", CLIP_PIECE_DEFAULT, pieces))) return rc;
        // [0, 8): the totals; [8, 8 + 528): the cells; [536]: the bad bounds row
        unsigned long long *d_total = arena_new<unsigned long long>(c, CLIP_TOTALS + CLIP_CELLS + 1); if (!d_total) return NAF_GPU_ENOMEM;
        unsigned long long *d_cells = d_total + CLIP_TOTALS, *d_bad = d_cells + CLIP_CELLS;
        u64 *win = arena_new<u64>(c, 2 * count); u32 *wflags = arena_new<u32>(c, count);
        if (!win || !wflags) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(d_total, 0, (CLIP_TOTALS + CLIP_CELLS) * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
        LAUNCH(c, "unnaf_clip_stage", k_bounds_stage, (u32)((count + 255) / 256), 256, 0, d_bounds, 40u, 32u, (u32)NAF_GPU_TRIM_ERRORS, P.rec_base, first, count, win, wflags, (u8 *)nullptr, d_bad);
        PieceSweep sw(c, d_naf, pl, who);                                             // (behind the tables of the whole call: they stay when a piece is released)
        for (const RecPiece &pc : pieces) {
            const u64 nr = pc.r_hi - pc.r_lo;
            unsigned long long *keys = arena_new<unsigned long long>(c, nr); if (!keys) return NAF_GPU_ENOMEM;
            HIP_TRY(c, hipMemsetAsync(keys, 0xFF, nr * 8, c->stream));
            if (pc.p_hi > pc.p_lo) {
                PieceSweep::Tiles tl;
                if ((rc = sw.seq_for(pc, CLIP_TILE, &tl))) return rc;
                if (any_long) LAUNCH(c, "unnaf_clip_mark", (k_clip_mark<true>), (u32)tl.ntiles, 64, 0, Q, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, (const u64 *)(win + 2 * (pc.r_lo - first)), keys);
                else LAUNCH(c, "unnaf_clip_mark", (k_clip_mark<false>), (u32)tl.ntiles, 64, 0, Q, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, (const u64 *)(win + 2 * (pc.r_lo - first)), keys);
            }
            ClipFinP F; memset(&F, 0, sizeof F);
            F.rec_base = P.rec_base; F.win = win + 2 * (pc.r_lo - first); F.wflags = wflags + (pc.r_lo - first); F.keys = keys;
            F.r_lo = pc.r_lo; F.r_hi = pc.r_hi; F.min_len = o->min_len; F.total = d_total; F.cells = d_cells;
            memcpy(F.len, Q.len, sizeof F.len);
            if (d_rows && (rc = rows_out(c, &F.rows, nr, CLIP_ROW_U64))) return rc;
            LAUNCH(c, "unnaf_clip_finish", k_clip_finish, (u32)((nr + 255) / 256), 256, 0, F);
            if (d_rows) rows_copy(c, "unnaf_clip_copy", F.rows, d_rows + 40 * (pc.r_lo - first), nr, CLIP_ROW_U64, d_bad);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            sw.release();
        }
        std::vector<u64> sum(CLIP_TOTALS + CLIP_CELLS + 1);
        if ((rc = ctx_readback(c, sum.data(), d_total, sum.size() * 8))) return rc;
        const u64 bad = sum[CLIP_TOTALS + CLIP_CELLS];
        if (bad != BOUNDS_OK) { *n_records = 0; return bounds_row_fail(c, who, bad); }
        if (h_total) { h_total->reads = sum[0]; h_total->clipped = sum[1]; h_total->kept = sum[2]; h_total->bases = sum[3]; h_total->kept_bases = sum[4];
                       h_total->removed_bases = sum[5]; h_total->n_short = sum[6]; h_total->n_errors = sum[7]; }
        if (per_adapter) for (size_t k = 0; k < 33 * n_adapters; k++) per_adapter[k] = sum[CLIP_TOTALS + k];
        if (ctx_tracing(c)) ctx_trace(c, "[clip] adapters %zu records %llu clipped %llu pieces %zu sequence bytes decoded %llu of %llu\n", n_adapters, (unsigned long long)count,
                                      (unsigned long long)sum[1], pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes);
        return 0;
    };
    rc = run();
    if (rc && h_total) memset(h_total, 0, sizeof *h_total);
    arena_settle(c);
    return rc;
}
