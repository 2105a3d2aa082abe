// composition.h -- base composition per record and per window, counted in the packed 4-bit stream (naf_gpu_composition_rows_of,
// naf_gpu_unnaf_composition_rows, naf_gpu_unnaf_composition).  Part of emit.hip (included by it, behind locate.h): the front of the
// call, the pieces and the decode of a piece's bytes are payload.h's (records_front, piece_plan, PieceSweep); the lane's 64 bases, the base
// behind them, the bit planes and the row copy are packed.h's; this file holds the row tables, the counting kernels and their launches.
//
// The contract (include/naf_gpu.h carries it too):
//   rows      window 0: one row per record, [0, len), an empty record a row of zeros.  window W > 0: ceil(len / W) rows
//             [k W, min((k + 1) W, len)) per record, an empty record none.  Ascending (record, begin); sum(n[0..15]) == end - begin.
//   n[c]      stored bases with 4-bit code c ("-TGKCYSBAWRDMHVN").  Bases behind the last record of a malformed archive and the padding
//             nibble of an odd stream are in no row.
//   cpg       positions g of the row with base g == C (4) and base g + 1 == G (2), g + 1 in the same record (it may lie in the next window).
//   masked    bases g of the row with an odd number of mask toggles <= g (g counts through the whole stream); 0 without the flag or
//             without a mask section, and the mask is then not decoded.
//
// A row is 21 u64: record, begin, end, n[16], masked, cpg.  row_base[r] is the exclusive scan of rows_of(rec_len[r], W), so every row's
// place is known before anything is decoded and one sweep over the packed bytes is enough.  k_comp_rows (a lane per row) zeroes the rows,
// writes record / begin / end and takes `masked` from the toggles: ex[k] = masked bases in front of toggle k - 1 (a scan over the toggle
// list), so the masked bases in front of any position are one upper_bound, and a row is the difference of two.  k_comp_count (a wavefront
// per tile of 4096 bases, 64 bases a lane as two 16-byte loads, tiles start on an even base as in k_locate) counts by bit planes: the four
// planes of a dword's eight nibbles are (x >> b) & 0x11111111, a code is an AND of planes or of their complements, v_bcnt_u32_b32 adds up.
// A tile whose counted codes are all single nucleotides (a ballot) needs the four planes' popcounts only; the general path builds the
// sixteen ANDs from two groups of four.  CpG is C_plane & (G_plane moved down one nibble); the base behind a lane's last comes from the
// neighbour lane, behind the tile's last from one bounds-checked byte, and the C's are cut one base in front of the record's end.
// A lane whose bases lie in one row keeps its counts in registers; lanes of the same row are summed across the wave (two rounds: the
// row the tile starts in and the next one) and ONE lane issues an atomic per non-zero counter; what is left, and lanes that straddle
// row or record ends (counted part by part under nibble masks), add their own.  Integer adds: the result does not depend on the order.
// Atomics need 8-byte alignment: a d_rows that has it is counted in place, any other gets the rows of a piece from an arena copy.
#pragma once

#define COMP_TILE 4096u
#define COMP_ROW_U64 21u
#define COMP_PIECE_DEFAULT (1ull << 31)      // bases counted per decode (NAF_GPU_COMPOSITION_PIECE)

__host__ __device__ __forceinline__ u64 comp_rows_of(u64 n, u64 W) { return W == 0 ? 1 : n / W + (n % W != 0); }

// bit 0 of every nibble of dword i (bases 8 i .. 8 i + 7 of a lane) whose base number is < k, k in 0 .. 64
__device__ __forceinline__ u32 comp_below(u32 k, int i)
{
    const int kk = (int)k - 8 * i;
    return kk <= 0 ? 0u : kk >= 8 ? NIB_L : (NIB_L & ((1u << (4 * kk)) - 1u));
}

// Counts of a lane's bases [a, b) into cnt[0..15], and into cnt[16] the C's of [a, bc) (bc <= b) whose next base is a G.  x: the lane's 64
// nibbles; gnext: 1 when the base behind the lane's last is a G.  FAST: every base of [a, b) -- and every base behind a C of [a, bc) that
// lies in this lane -- is a single nucleotide, so a plane IS a letter.  FULL: a = 0, b = bc = 64.
template <bool FAST, bool FULL>
__device__ __forceinline__ void comp_span(const u32 (&x)[8], u32 gnext, u32 a, u32 b, u32 bc, u32 (&cnt)[17])
{
    u32 g2[9];
#pragma unroll
    for (int i = 0; i < 8; i++) { const u32 y = x[i]; g2[i] = FAST ? (y >> 1) & NIB_L : ~y & (y >> 1) & ~(y >> 2) & ~(y >> 3) & NIB_L; }
    g2[8] = gnext;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 m = FULL ? NIB_L : comp_below(b, i) & ~comp_below(a, i), mc = FULL ? NIB_L : comp_below(bc, i) & ~comp_below(a, i);
        const u32 gn = (g2[i] >> 4) | (g2[i + 1] << 28);
        if (FAST) {
            const u32 y = x[i], p2 = (y >> 2) & NIB_L;
            cnt[1] += __popc(y & NIB_L & m); cnt[2] += __popc((y >> 1) & NIB_L & m); cnt[4] += __popc(p2 & m); cnt[8] += __popc((y >> 3) & NIB_L & m);
            cnt[16] += __popc(p2 & gn & mc);
        } else {
            u32 lo[4], hi[4]; nib_products(x[i], lo, hi);
#pragma unroll
            for (int l = 0; l < 4; l++) lo[l] &= m;
#pragma unroll
            for (int h = 0; h < 4; h++)
#pragma unroll
                for (int l = 0; l < 4; l++) cnt[4 * h + l] += __popc(lo[l] & hi[h]);
            cnt[16] += __popc(lo[0] & hi[1] & gn & mc);
        }
    }
}
__device__ __forceinline__ void comp_flush(u64 *row, const u32 (&cnt)[17])
{
#pragma unroll
    for (int k = 0; k < 16; k++) if (cnt[k]) atomicAdd((unsigned long long *)row + 3 + k, (unsigned long long)cnt[k]);
    if (cnt[16]) atomicAdd((unsigned long long *)row + 20, (unsigned long long)cnt[16]);
}

// seq: pointer to packed byte 0 of the stream; bytes [.., b_end) of it may be read.  Records [r_lo, r_hi) are counted: rec_base[r_lo] = p_lo,
// rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.  row_base[r - first]: first row of record r; acc: row R0 (21 u64 a row,
// 8-byte aligned, zeroed by k_comp_rows).  paths (may be null): tiles counted by the nucleotide path / by the general path.
__global__ __launch_bounds__(64) void k_comp_count(const u8 *seq, u64 b_end, const u64 *rec_base, const u64 *row_base, u64 first, u64 r_lo, u64 r_hi,
                                                   u64 p_lo, u64 p_hi, u64 t0, u64 W, u64 R0, u64 *acc, unsigned long long *paths)
{
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    const u64 g = t0 + t * COMP_TILE + lane * 64;                                 // the lane's first base
    const u64 lo = g > p_lo ? g : p_lo, hi = g + 64 < p_hi ? g + 64 : p_hi;       // the bases of it that are counted
    const bool active = g < p_hi && lo < hi;
    u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (active) packed_load64(seq, b_end, g, x);
    const u32 gnext = packed_behind(seq, b_end, g, active, lane, x) == 2u ? 1u : 0u;

    // single nucleotides only?  the sum of the planes is the number of letters in a base's set
    const u32 a0 = active ? (u32)(lo - g) : 0u, b0n = active ? (u32)(hi - g) : 0u;
    u32 bad = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 y = x[i], s = (y & NIB_L) + ((y >> 1) & NIB_L) + ((y >> 2) & NIB_L) + ((y >> 3) & NIB_L);
        bad |= (s ^ NIB_L) & ((comp_below(b0n, i) & ~comp_below(a0, i)) * 15u);
    }
    const bool fast = __ballot(bad != 0) == 0;
    if (paths && lane == 0) atomicAdd(&paths[fast ? 0 : 1], 1ull);

    u32 cnt[17];
#pragma unroll
    for (int k = 0; k < 17; k++) cnt[k] = 0;
    bool pending = false; u64 myrow = 0;
    if (active) {
        u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, lo) - 1;                // rec_base[r] <= lo < rec_base[r + 1]
        u64 rbase = rec_base[r], rend = rec_base[r + 1];
        bool one = W == 0 || rend - rbase <= W;                                   // the record is one row
        u64 k = one ? 0 : (lo - rbase) / W;
        u64 row = row_base[r - first] + k;
        u64 rowend = one || rend - rbase - k * W <= W ? rend : rbase + k * W + W;
        if (hi <= rowend && lo == g && hi == g + 64 && rend - 1 >= hi) {          // the normal case: all 64 bases in one row, the next base in the same record
            if (fast) comp_span<true, true>(x, gnext, 0, 64, 64, cnt); else comp_span<false, true>(x, gnext, 0, 64, 64, cnt);
            pending = true; myrow = row;
        } else {
            u64 at = lo;
            for (;;) {                                                            // part by part under nibble masks
                const u64 e = hi < rowend ? hi : rowend, ce = e < rend - 1 ? e : rend - 1;
                // (the planes and their products do not depend on the part: left alone, the compiler computes all 128 of them in front
                // of the loop and keeps them -- 212 VGPRs; the bases are made opaque so that every part computes what it needs)
#pragma unroll
                for (int q = 0; q < 8; q++) asm volatile("" : "+v"(x[q]));
                if (fast) comp_span<true, false>(x, gnext, (u32)(at - g), (u32)(e - g), (u32)(ce - g), cnt);
                else comp_span<false, false>(x, gnext, (u32)(at - g), (u32)(e - g), (u32)(ce - g), cnt);
                if (at == lo && e == hi) { pending = true; myrow = row; break; }  // one row after all: kept for the wave's sum
                comp_flush(acc + (row - R0) * COMP_ROW_U64, cnt);
#pragma unroll
                for (int q = 0; q < 17; q++) cnt[q] = 0;
                at = e;
                if (at >= hi) break;
                if (at >= rend) {                                                 // the next record that has bases (at < hi <= p_hi: there is one)
                    do { r++; rbase = rend; rend = rec_base[r + 1]; } while (rend <= at);
                    one = W == 0 || rend - rbase <= W; k = 0; row = row_base[r - first];
                } else { k++; row++; }
                rowend = one || rend - rbase - k * W <= W ? rend : rbase + k * W + W;
            }
        }
    }
    // lanes of one row: summed across the wave, one lane adds.  Two rounds cover a tile that lies in one row or in two.
#pragma unroll 1
    for (int it = 0; it < 2; it++) {
        const u64 pend = __ballot(pending);
        if (!pend) break;
        const int leader = __ffsll((long long)pend) - 1;
        const u64 lrow = shfl_u64(myrow, leader);
        const bool in = pending && myrow == lrow;
        u64 *o = acc + (lrow - R0) * COMP_ROW_U64;
        const bool lead = (int)lane == leader;
#define COMP_SUM(k) do { const u32 v = wave_sum_u32(in ? cnt[k] : 0u); if (lead && v) atomicAdd((unsigned long long *)o + ((k) < 16 ? 3 + (k) : 20), (unsigned long long)v); } while (0)
        if (fast) { COMP_SUM(1); COMP_SUM(2); COMP_SUM(4); COMP_SUM(8); COMP_SUM(16); }
        else {
#pragma unroll
            for (int k = 0; k < 17; k++) COMP_SUM(k);
        }
#undef COMP_SUM
        pending = pending && !in;
    }
    if (pending) comp_flush(acc + (myrow - R0) * COMP_ROW_U64, cnt);
}

// out[i] = rows of record first + i, i < n; out[n] = 0 (the scan's total lands there)
__global__ __launch_bounds__(256) void k_comp_rowcount(const u64 *rec_len, u64 n, u64 W, u64 *out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) out[i] = i < n ? comp_rows_of(rec_len[i], W) : 0;
}
// val[i] = masked bases between toggle i - 1 and toggle i (odd i), 0 for even i and for i = n
__global__ __launch_bounds__(256) void k_comp_togval(const u64 *tg, u64 n, u64 *val)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) val[i] = (i < n && (i & 1)) ? tg[i] - tg[i - 1] : 0;
}
// masked bases in front of position x: ex[k] = masked bases in front of toggle k - 1
__device__ __forceinline__ u64 comp_masked_below(const u64 *tg, const u64 *ex, u64 n, u64 x)
{
    if (x == 0) return 0;
    const u64 k = upper_bound_u64(tg, 0, n, x - 1);                               // toggles < x
    return k == 0 ? 0 : ex[k] + ((k & 1) ? x - tg[k - 1] : 0);
}
// a lane per row R0 + j, j < nrows: zeroes it, writes record, begin, end and masked
__global__ __launch_bounds__(256) void k_comp_rows(const u64 *rec_base, const u64 *row_base, u64 first, u64 r_lo, u64 r_hi, u64 R0, u64 nrows, u64 W,
                                                   const u64 *tg, const u64 *ex, u64 n_tog, u64 *acc)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nrows) return;
    const u64 ri = upper_bound_u64(row_base, r_lo - first, r_hi - first + 1, R0 + j) - 1;      // the last record whose rows start at or before this one: the one that has it
    const u64 k = R0 + j - row_base[ri], base = rec_base[first + ri], len = rec_base[first + ri + 1] - base;
    const u64 begin = W ? k * W : 0, end = (W && len - begin > W) ? begin + W : len;
    u64 *o = acc + j * COMP_ROW_U64;
    o[0] = first + ri; o[1] = begin; o[2] = end;
#pragma unroll
    for (int q = 3; q < 21; q++) o[q] = 0;
    if (ex) o[19] = comp_masked_below(tg, ex, n_tog, base + end) - comp_masked_below(tg, ex, n_tog, base + begin);
}
// total[0..17] += n[16], masked, cpg of the rows
__global__ __launch_bounds__(256) void k_comp_total(const u64 *acc, u64 nrows, unsigned long long *total)
{
    u64 s[18];
#pragma unroll
    for (int q = 0; q < 18; q++) s[q] = 0;
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < nrows; j += (u64)gridDim.x * 256) {
#pragma unroll
        for (int q = 0; q < 18; q++) s[q] += acc[j * COMP_ROW_U64 + 3 + q];
    }
#pragma unroll
    for (int q = 0; q < 18; q++) {
        const u64 v = wave_sum_u64(s[q]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&total[q], (unsigned long long)v);
    }
}
// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" uint64_t naf_gpu_composition_rows_of(uint64_t n_bases, uint64_t window) { return comp_rows_of(n_bases, window); }

static int composition_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, u64 W, int flags, u64 first, u64 count, u8 *d_rows, size_t row_cap,
                           u64 *n_rows, naf_gpu_comp_row *h_total, bool rows_only)
{
    if (!c || !d_naf || !n_rows) return NAF_GPU_EARG;
    *n_rows = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    if (flags & ~(int)NAF_GPU_COMP_MASK) return ctx_fail(c, NAF_GPU_EARG, "composition: flags %d: only bit 0 (NAF_GPU_COMP_MASK) is defined", flags);
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT | (!rows_only && (flags & NAF_GPU_COMP_MASK) ? FRONT_MASK : 0), "composition", "nucleotides cannot be counted", first, &count, pl);   // the mask only when asked for
    if (rc || !count) return rc;
    const EmitP &P = pl.P;

    // every row's place: row_base[i] = first row of record first + i, row_base[count] = rows in all
    LAUNCH_LIMIT(c, count + 1, 1, "composition: %llu records are too many for one launch", (unsigned long long)count);
    u64 *row_base = arena_new<u64>(c, count + 2); if (!row_base) return NAF_GPU_ENOMEM;
    LAUNCH(c, "unnaf_comp_rowcount", k_comp_rowcount, (u32)((count + 256) / 256), 256, 0, P.rec_len + first, count, W, row_base);
    if ((rc = scan_exclusive_u64(c, row_base, count + 1, (u64 *)nullptr))) return rc;
    u64 total = 0;
    if ((rc = ctx_readback(c, &total, row_base + count, 8))) return rc;
    *n_rows = total;
    if (rows_only) return 0;
    if (total > row_cap) return ctx_fail(c, NAF_GPU_ECAP, "composition: %llu rows, capacity %zu", (unsigned long long)total, row_cap);
    // the pieces, and the first row of every piece (and the end of the last)
    std::vector<RecPiece> pieces;
    std::vector<u64> rows_at;
    if ((rc = piece_plan(c, P, first, count, "COMPOSITION_PIECE", COMP_PIECE_DEFAULT, pieces, row_base, total, &rows_at))) return rc;
    if (h_total) { h_total->record = count; h_total->end = pieces.back().p_hi - pieces.front().p_lo; }
    if (total == 0) return 0;
    if (!d_rows) return ctx_fail(c, NAF_GPU_EARG, "composition: no place for the rows (d_rows is NULL)");

    // masked bases in front of every toggle
    const u64 *tog_ex = nullptr;
    if (P.masking && P.n_toggles) {
        LAUNCH_LIMIT(c, P.n_toggles + 1, 1, "composition: %llu mask toggles are too many for one launch", (unsigned long long)P.n_toggles);
        u64 *ex = arena_new<u64>(c, P.n_toggles + 2); if (!ex) return NAF_GPU_ENOMEM;
        LAUNCH(c, "unnaf_comp_mask", k_comp_togval, (u32)((P.n_toggles + 256) / 256), 256, 0, P.toggles, P.n_toggles, ex);
        if ((rc = scan_exclusive_u64(c, ex, P.n_toggles + 1, (u64 *)nullptr))) return rc;
        tog_ex = ex;
    }
    u64 *d_sum = arena_new<u64>(c, 20); if (!d_sum) return NAF_GPU_ENOMEM;      // [0..17] the total, [18] / [19] tiles of the two paths
    HIP_TRY(c, hipMemsetAsync(d_sum, 0, 20 * 8, c->stream));
    const bool tracing = ctx_tracing(c), in_place = ((uintptr_t)d_rows & 7) == 0;

    PieceSweep sw(c, d_naf, pl, "composition");
    for (size_t pi = 0; pi < pieces.size(); pi++) {
        const RecPiece &pc = pieces[pi];
        const u64 R0 = rows_at[pi], nr = rows_at[pi + 1] - R0;
        if (!nr) continue;
        LAUNCH_LIMIT(c, nr, COMP_ROW_U64, "composition: a piece of %llu rows is too long for one launch", (unsigned long long)nr);
        const bool bases = pc.p_hi > pc.p_lo;                                     // (empty records at window 0: rows, and nothing to decode)
        PieceSweep::Tiles tl = {};
        if (bases && (rc = sw.seq_for(pc, COMP_TILE, &tl))) return rc;
        u64 *acc = in_place ? (u64 *)(d_rows + 168 * R0) : arena_new<u64>(c, nr * COMP_ROW_U64);
        if (!acc) return NAF_GPU_ENOMEM;
        LAUNCH(c, "unnaf_comp_rows", k_comp_rows, (u32)((nr + 255) / 256), 256, 0, P.rec_base, (const u64 *)row_base, first, pc.r_lo, pc.r_hi, R0, nr, W,
               P.toggles, tog_ex, P.n_toggles, acc);
        if (bases) LAUNCH(c, "unnaf_comp_count", k_comp_count, (u32)tl.ntiles, 64, 0, tl.seq, tl.b_hi, P.rec_base, (const u64 *)row_base, first, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, W, R0, acc,
                          tracing ? (unsigned long long *)d_sum + 18 : (unsigned long long *)nullptr);
        if (h_total) { const u64 nb = (nr + 255) / 256; LAUNCH(c, "unnaf_comp_total", k_comp_total, (u32)(nb < 2048 ? nb : 2048), 256, 0, (const u64 *)acc, nr, (unsigned long long *)d_sum); }
        if (!in_place) rows_copy(c, "unnaf_row_copy", acc, d_rows + 168 * R0, nr, COMP_ROW_U64);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        sw.release();
    }
    u64 sum[20];
    if (h_total || tracing) { if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc; }
    if (h_total) { for (int k = 0; k < 16; k++) h_total->n[k] = sum[k]; h_total->masked = sum[16]; h_total->cpg = sum[17]; }
    if (tracing) ctx_trace(c, "[composition] rows %llu window %llu pieces %zu sequence bytes decoded %llu of %llu mask %llu tiles nucleotide %llu general %llu\n", (unsigned long long)total,
                           (unsigned long long)W, pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes, (unsigned long long)(tog_ex ? P.n_toggles : 0),
                           (unsigned long long)sum[18], (unsigned long long)sum[19]);
    return 0;
}

extern "C" int naf_gpu_unnaf_composition_rows(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t window, uint64_t first, uint64_t count, uint64_t *n_rows)
{
    int rc = composition_run(c, (const u8 *)d_naf, naf_len, window, 0, first, count, nullptr, 0, n_rows, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_composition(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t window, int flags, uint64_t first, uint64_t count,
                                         naf_gpu_comp_row *d_rows, size_t row_cap, uint64_t *n_rows, naf_gpu_comp_row *h_total)
{
    int rc = composition_run(c, (const u8 *)d_naf, naf_len, window, flags, first, count, (u8 *)d_rows, row_cap, n_rows, h_total, false);
    if (c) arena_settle(c);
    return rc;
}
