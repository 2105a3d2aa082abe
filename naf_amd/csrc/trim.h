// trim.h -- quality trimming and filtering of reads, decided in the quality stream (naf_gpu_trim_limit, naf_gpu_unnaf_trim).  Part of
// emit.hip (included by it, behind repeats.h): the front of the call, the pieces and the decode of a piece's bytes are quality.h's and
// payload.h's (quality_front, piece_plan, PieceSweep), the row copy is packed.h's; this file holds the summaries, the two kernels and
// their launches.  The contract is include/naf_gpu.h's.
//
// A quality byte b scores s(b) = limit - tab[b] (64-bit integers).  The stretch of a read is its interval of the largest positive score
// sum, the smallest begin among equal sums, then the largest end.  That order makes the rule a combine of SUMMARIES of neighbouring
// pieces of a read -- (total, best prefix: sum and end, best suffix: sum and begin, best: sum, begin, end), the empty prefix and the
// empty suffix (sum 0) among the candidates, prefix ties to the larger end, suffix ties to the smaller begin, the cross candidate the
// left suffix plus the right prefix -- and the combine is associative, so the pieces can be cut anywhere (trim_combine).  Positions are
// stream byte indices (in a tile: relative to the tile's first byte, 32 bits), so a summary needs no length.
//
// k_trim_mark: a workgroup of four wavefronts, a wavefront per tile of 4096 quality bytes, 64 bytes a lane as four 16-byte loads; tiles
// start where the ADDRESS is a multiple of 16, as in k_qual_count, and lanes whose 64 bytes do not lie inside the decoded range load byte
// by byte.  A lane puts its bytes into a row of its own in LDS (17 dwords a lane: the lanes' byte reads fall into different banks) and
// walks them ONCE, part by part (lane_parts), one read of the 256-entry score table a byte.  A part that is a whole record writes its row;
// the others go through seam_carry, and the first lane of a record then holds the summary of all bytes the record has in the tile: a
// record that lies inside the tile gets its row, one that began in front of the tile leaves the summary in slot 0 of the tile, one that
// begins in it and ends behind it in slot 1 (open[2 * ntiles]).
//
// k_trim_join: a lane per record of the piece.  An empty record writes its row (never kept: an empty stretch is short); a record whose
// bytes touch more than one tile gets its summary from seam_join and writes its row; the others return.  A record of 2^31 bytes costs
// its lane 2^19 steps.
//
// Every row is written by exactly one lane, into a table in the arena (5 u64 a row) that rows_copy takes to the caller's, whatever its
// alignment.  The totals go through wg_sums.  Nothing depends on the tile origin or on the piece size.
#pragma once

#define TRIM_TILE 4096u
#define TRIM_ROW_U64 5u
#define TRIM_LANE_DWORDS 17u                    // a lane's row of the staging table: its 64 bytes and one dword to spread the banks
#define TRIM_PIECE_DEFAULT (1ull << 31)        // quality bytes swept per decode (NAF_GPU_TRIM_PIECE)
#define TRIM_TOTALS 8u                          // reads, kept, bases, kept_bases, kept_ee, n_short, n_errors; [7]: tile slots joined (the trace)

template <typename POS>
struct TrimSum { i64 tot, pre, suf, best; POS pre_end, suf_begin, b, e; };       // best == 0: no interval of positive sum (b = e = 0)
typedef TrimSum<u32> TrimSum32;
typedef TrimSum<u64> TrimOpen;                  // a tile's slot: positions as stream byte indices (64 bytes)

// the summary of no bytes at position p
__device__ __forceinline__ TrimSum32 trim_empty(u32 p) { TrimSum32 S; S.tot = S.pre = S.suf = S.best = 0; S.pre_end = S.suf_begin = p; S.b = S.e = 0; return S; }
// The summary of bytes [.., p) becomes that of [.., p + 1): the byte at p scores s.  (trim_combine with a one-byte summary, written out.)
// last: the best interval's LAST byte, end - 1 -- with the end itself the compiler folds the two stores of p + 1 into one through a
// pointer, and both variables then live in scratch memory.
__device__ __forceinline__ void trim_append(i64 &tot, i64 &pre, i64 &suf, i64 &best, u32 &pre_end, u32 &suf_begin, u32 &b, u32 &last, u32 p, i64 s)
{
    tot += s;
    if (tot >= pre) { pre = tot; pre_end = p + 1; }                              // the longer prefix wins a tie
    const i64 t = suf + s;
    if (t >= 0) {                                                                 // the suffix goes on (the smaller begin wins a tie) and is the one new candidate
        suf = t;
        if (s >= 0 && t > 0 && (t > best || (t == best && suf_begin <= b))) { best = t; b = suf_begin; last = p; }
    } else { suf = 0; suf_begin = p + 1; }
}
// L's bytes, then R's
template <typename POS>
__device__ __forceinline__ TrimSum<POS> trim_combine(const TrimSum<POS> &L, const TrimSum<POS> &R)
{
    TrimSum<POS> o;
    o.tot = L.tot + R.tot;
    const i64 ps = L.tot + R.pre, ss = L.suf + R.tot, cs = L.suf + R.pre;
    if (ps >= L.pre) { o.pre = ps; o.pre_end = R.pre_end; } else { o.pre = L.pre; o.pre_end = L.pre_end; }
    if (ss >= R.suf) { o.suf = ss; o.suf_begin = L.suf_begin; } else { o.suf = R.suf; o.suf_begin = R.suf_begin; }
    if (R.best > L.best) { o.best = R.best; o.b = R.b; o.e = R.e; } else { o.best = L.best; o.b = L.b; o.e = L.e; }
    if (cs > 0 && (cs > o.best || (cs == o.best && (L.suf_begin < o.b || (L.suf_begin == o.b && R.pre_end > o.e))))) { o.best = cs; o.b = L.suf_begin; o.e = R.pre_end; }
    return o;
}
__device__ __forceinline__ TrimSum32 trim_sum_down(const TrimSum32 &S, int d)
{
    TrimSum32 o;
    o.tot = (i64)shfl_down_u64((u64)S.tot, d); o.pre = (i64)shfl_down_u64((u64)S.pre, d); o.suf = (i64)shfl_down_u64((u64)S.suf, d); o.best = (i64)shfl_down_u64((u64)S.best, d);
    o.pre_end = (u32)__shfl_down((int)S.pre_end, d); o.suf_begin = (u32)__shfl_down((int)S.suf_begin, d); o.b = (u32)__shfl_down((int)S.b, d); o.e = (u32)__shfl_down((int)S.e, d);
    return o;
}
__device__ __forceinline__ TrimOpen trim_open_of(const TrimSum32 &S, u64 T0)
{
    TrimOpen o; o.tot = S.tot; o.pre = S.pre; o.suf = S.suf; o.best = S.best;
    o.pre_end = T0 + S.pre_end; o.suf_begin = T0 + S.suf_begin; o.b = T0 + S.b; o.e = T0 + S.e;
    return o;
}

struct TrimP {
    const u8 *q; u64 b_lo, b_hi;               // pointer to byte 0 of the quality stream; bytes [b_lo, b_hi) of it may be read
    const u64 *rec_base;                       // records [r_lo, r_hi) are swept: rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi
    u64 r_lo, r_hi, p_lo, p_hi;
    u64 t0, ntiles;                            // first byte of tile 0 (b_lo <= t0 <= p_lo), tiles that reach p_hi
    u64 limit; u32 none;                       // the cutoff; none: no trimming (limit = 0 then: the scores are -tab[b], their total is -ee)
    u64 min_len, max_ee;
    u64 *rows;                                 // row of record r_lo (5 u64 a row, 8-byte aligned), null: not wanted
    TrimOpen *open;                            // two slots a tile
    unsigned long long *total;                 // TRIM_TOTALS counters
};
typedef u64 TrimTot[TRIM_TOTALS];

// The row of record r = bytes [rbase, rend) of the stream, from the summary of all its bytes (positions: stream byte indices), and its
// share of the totals.
__device__ __forceinline__ void trim_row(const TrimP &P, u64 r, u64 rbase, u64 rend, i64 tot, i64 best, u64 b, u64 e, TrimTot &T)
{
    const u64 n = rend - rbase;
    u64 begin = 0, end = 0, ee = 0;
    if (P.none) { end = n; ee = (u64)(-tot); }
    else if (best > 0) { begin = b - rbase; end = e - rbase; ee = (end - begin) * P.limit - (u64)best; }
    const bool is_short = end - begin < P.min_len, errors = ee > P.max_ee;
    const u32 flags = is_short || errors ? (is_short ? NAF_GPU_TRIM_SHORT : 0u) | (errors ? NAF_GPU_TRIM_ERRORS : 0u) : NAF_GPU_TRIM_KEPT;
    if (P.rows) { u64 *o = P.rows + (r - P.r_lo) * TRIM_ROW_U64; o[0] = r; o[1] = begin; o[2] = end; o[3] = ee; o[4] = flags; }
    T[0]++; T[2] += n;
    if (flags == NAF_GPU_TRIM_KEPT) { T[1]++; T[3] += end - begin; T[4] += ee; }
    T[5] += is_short; T[6] += errors;
}

__global__ __launch_bounds__(256) void k_trim_mark(TrimP P)
{
    __shared__ i64 stab[256];
    __shared__ u32 stage[4][64 * TRIM_LANE_DWORDS];
    __shared__ unsigned long long tsum[TRIM_TOTALS];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    stab[tid] = (i64)P.limit - (i64)qual_err_of(qual_err_33_dev, tid);
    if (tid < TRIM_TOTALS) tsum[tid] = 0;
    __syncthreads();
    TrimTot T; for (u32 k = 0; k < TRIM_TOTALS; k++) T[k] = 0;
    const u64 tile = (u64)xcd_block() * 4 + wave;
    if (tile < P.ntiles) {                                                        // (the same for all lanes of a wave)
        const u64 T0 = P.t0 + tile * TRIM_TILE, g = T0 + lane * 64;               // the tile's and the lane's first byte
        const u64 lo = g > P.p_lo ? g : P.p_lo, hi = g + 64 < P.p_hi ? g + 64 : P.p_hi;   // the bytes of it that are swept
        const bool active = lo < hi;
        u32 *st = stage[wave] + lane * TRIM_LANE_DWORDS;
        TrimSum32 A = trim_empty(0), X = trim_empty(0);
        bool has_a = false, pend = false, thru = false;                          // A: a part that ends a record of the lane in front; X: one whose record goes on; thru: X came from there too
        u64 xr = 0, xbase = 0, xend = 0;                                          // X's record
        if (active) {
            if (g >= P.b_lo && g + 64 <= P.b_hi) {
#pragma unroll
                for (int i = 0; i < 4; i++) { u32x4 v; memcpy(&v, P.q + g + 16 * i, 16); st[4 * i] = v.x; st[4 * i + 1] = v.y; st[4 * i + 2] = v.z; st[4 * i + 3] = v.w; }
            } else {                                                              // the head or the tail of what was decoded
                for (int i = 0; i < 16; i++) {
                    u32 w = 0;
                    for (int j = 0; j < 4; j++) if (g + 4 * i + j >= lo && g + 4 * i + j < hi) w |= (u32)P.q[g + 4 * i + j] << (8 * j);
                    st[i] = w;
                }
            }
            const u8 *sb = (const u8 *)st;                                        // (read by the lane that wrote them: no barrier)
            const u32 g32 = lane * 64;
            lane_parts(P.rec_base, P.r_lo, P.r_hi, lo, hi, [&](u64 r, u64 rbase, u64 rend, u64 at64, u64 stop64) {
                const u32 at = (u32)(at64 - T0), stop = (u32)(stop64 - T0);         // the part: bytes [at, stop) of the tile
                i64 tot = 0, pre = 0, suf = 0, best = 0; u32 pre_end = at, suf_begin = at, bb = 0, last = 0;
#pragma unroll 1
                for (u32 pos = at; pos < stop; pos++) trim_append(tot, pre, suf, best, pre_end, suf_begin, bb, last, pos, stab[sb[pos - g32]]);
                TrimSum32 S; S.tot = tot; S.pre = pre; S.suf = suf; S.best = best; S.pre_end = pre_end; S.suf_begin = suf_begin; S.b = bb; S.e = best > 0 ? last + 1 : 0;
                const bool from_front = rbase < at64, goes_on = rend > stop64;
                if (!from_front && !goes_on) trim_row(P, r, rbase, rend, S.tot, S.best, T0 + S.b, T0 + S.e, T);
                else if (!goes_on) { A = S; has_a = true; }
                else { X = S; pend = true; thru = from_front; xr = r; xbase = rbase; xend = rend; }
            });
        }
        const bool head = seam_carry(lane, has_a, A, pend, thru, X, [](const TrimSum32 &S, int d) { return trim_sum_down(S, d); },
                                     [](const TrimSum32 &L, const TrimSum32 &R) { return trim_combine(L, R); });
        if (lane == 0 && has_a) P.open[2 * tile] = trim_open_of(A, T0);          // it came from the tile in front: the record's bytes in this tile are that part
        if (head) {
            if (xbase >= T0 && xend <= T0 + TRIM_TILE) trim_row(P, xr, xbase, xend, X.tot, X.best, T0 + X.b, T0 + X.e, T);
            else P.open[2 * tile + (xbase < T0 ? 0 : 1)] = trim_open_of(X, T0);
        }
    }
    wg_sums(T, tsum, P.total);
}

__global__ __launch_bounds__(256) void k_trim_join(TrimP P)
{
    __shared__ unsigned long long tsum[TRIM_TOTALS];
    if (threadIdx.x < TRIM_TOTALS) tsum[threadIdx.x] = 0;
    __syncthreads();
    TrimTot T; for (u32 k = 0; k < TRIM_TOTALS; k++) T[k] = 0;
    const u64 r = P.r_lo + (u64)blockIdx.x * 256 + threadIdx.x;
    if (r < P.r_hi) {
        const u64 rbase = P.rec_base[r], rend = P.rec_base[r + 1];
        if (rend == rbase) trim_row(P, r, rbase, rend, 0, 0, 0, 0, T);
        else {
            TrimOpen S;
            const u64 tiles = seam_join(P.open, P.t0, TRIM_TILE, rbase, rend, S, [](const TrimOpen &L, const TrimOpen &R) { return trim_combine(L, R); });
            if (tiles > 1) { trim_row(P, r, rbase, rend, S.tot, S.best, S.b, S.e, T); T[7] += tiles; }
        }
    }
    wg_sums(T, tsum, P.total);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_trim_limit(unsigned phred, uint64_t *limit)
{
    if (!limit || phred > 93) return NAF_GPU_EARG;
    *limit = qual_err_33[phred];
    return 0;
}

extern "C" int naf_gpu_unnaf_trim(naf_gpu_ctx *c, const void *d_naf_, size_t naf_len, const naf_gpu_trim_opts *o, uint64_t first, uint64_t count,
                                  naf_gpu_trim_row *d_rows_, size_t row_cap, uint64_t *n_records, naf_gpu_trim_total *h_total)
{
    const u8 *d_naf = (const u8 *)d_naf_; u8 *d_rows = (u8 *)d_rows_;
    if (!c || !d_naf || !o || !n_records) return NAF_GPU_EARG;
    *n_records = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    const bool none = o->limit == NAF_GPU_TRIM_NONE;
    if (o->limit == 0 || (!none && o->limit > (1ull << 32)))
        return ctx_fail(c, NAF_GPU_EARG, "trim: limit %llu is no error rate times 2^32 (1 .. 4294967296, or NAF_GPU_TRIM_NONE)", (unsigned long long)o->limit);
    if (o->min_len == 0) return ctx_fail(c, NAF_GPU_EARG, "trim: min_len 0 (a kept read has at least one base)");
    UnnafPlan pl;
    int rc = quality_front(c, d_naf, naf_len, first, &count, pl);
    if (rc) { arena_settle(c); return rc; }
    *n_records = count;
    if (!count) { arena_settle(c); return 0; }
    auto run = [&]() -> int {
        const EmitP &P = pl.P;
        if (d_rows && count > row_cap) return cap_fail(c, "trim", "rows", count, row_cap);
        std::vector<RecPiece> pieces;
        if ((rc = piece_plan(c, P, first, count, "TRIM_PIECE", TRIM_PIECE_DEFAULT, pieces))) return rc;
        unsigned long long *d_total = arena_new<unsigned long long>(c, TRIM_TOTALS); if (!d_total) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(d_total, 0, TRIM_TOTALS * 8, c->stream));
        PieceSweep sw(c, d_naf, pl, "trim", S_QUAL);
        for (const RecPiece &pc : pieces) {
            const u64 nr = pc.r_hi - pc.r_lo;
            LAUNCH_LIMIT(c, nr, TRIM_ROW_U64, "trim: a piece of %llu records is too long for one launch", (unsigned long long)nr);
            TrimP Q; memset(&Q, 0, sizeof Q);
            Q.rec_base = P.rec_base; Q.r_lo = pc.r_lo; Q.r_hi = pc.r_hi; Q.p_lo = pc.p_lo; Q.p_hi = pc.p_hi;
            Q.limit = none ? 0 : o->limit; Q.none = none; Q.min_len = o->min_len; Q.max_ee = o->max_ee; Q.total = d_total;
            if (pc.p_hi > pc.p_lo) {
                PayloadSpan sp;
                if ((rc = sw.bytes_for(pc.p_lo, pc.p_hi, &sp))) return rc;
                Q.q = sp.base; Q.b_lo = sp.got_lo; Q.b_hi = sp.got_hi;
                if (Q.b_lo > pc.p_lo || Q.b_hi < pc.p_hi) return ctx_fail(c, NAF_GPU_EFORMAT, "can't decompress quality\n");
                const u64 mis = (u64)((uintptr_t)(Q.q + pc.p_lo) & 15u);          // tiles start on a 16-byte address when the decoded range reaches that far down
                Q.t0 = pc.p_lo - Q.b_lo >= mis ? pc.p_lo - mis : pc.p_lo;
                Q.ntiles = (pc.p_hi - Q.t0 + TRIM_TILE - 1) / TRIM_TILE;
                if (Q.ntiles > 0x7FFFFFFFull) return ctx_fail(c, NAF_GPU_EARG, "trim: a piece of %llu quality bytes is too long for one launch", (unsigned long long)(pc.p_hi - pc.p_lo));
            }
            if (d_rows && (rc = rows_out(c, &Q.rows, nr, TRIM_ROW_U64))) return rc;
            if (Q.ntiles) {
                Q.open = arena_new<TrimOpen>(c, 2 * Q.ntiles); if (!Q.open) return NAF_GPU_ENOMEM;
                LAUNCH(c, "unnaf_trim_mark", k_trim_mark, (u32)((Q.ntiles + 3) / 4), 256, 0, Q);
            }
            LAUNCH(c, "unnaf_trim_join", k_trim_join, (u32)((nr + 255) / 256), 256, 0, Q);
            if (d_rows) rows_copy(c, "unnaf_row_copy", Q.rows, d_rows + 40 * (pc.r_lo - first), nr, TRIM_ROW_U64);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            sw.release();
        }
        u64 sum[TRIM_TOTALS];
        if ((rc = ctx_readback(c, sum, d_total, sizeof sum))) return rc;
        if (h_total) { h_total->reads = sum[0]; h_total->kept = sum[1]; h_total->bases = sum[2]; h_total->kept_bases = sum[3]; h_total->kept_ee = sum[4]; h_total->n_short = sum[5]; h_total->n_errors = sum[6]; }
        if (ctx_tracing(c)) ctx_trace(c, "[trim] records %llu kept %llu pieces %zu quality bytes decoded %llu of %llu open tiles %llu\n", (unsigned long long)count, (unsigned long long)sum[1],
                                      pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.h.orig_size[S_QUAL], (unsigned long long)sum[7]);
        return 0;
    };
    rc = run();
    arena_settle(c);
    return rc;
}
