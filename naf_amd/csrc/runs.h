// runs.h -- runs of a base class and soft-masked intervals per record, listed from the packed 4-bit stream and from the mask's toggle
// list (naf_gpu_parse_base_class, naf_gpu_unnaf_runs_count, naf_gpu_unnaf_runs).  Part of emit.hip (included by it, behind quality.h):
// the front of the call, the pieces and the decode of a piece's bytes are payload.h's (records_front, piece_plan, PieceSweep); the lane's
// 64 bases, the bases in front of and behind them and the bit planes are packed.h's; this file holds the class parser, the kernels and
// their launches.
//
// The contract (include/naf_gpu.h carries it too):
//   class     bit c of `set` = 4-bit code c of "-TGKCYSBAWRDMHVN".  Membership is LITERAL: a stored N is in {N}, a stored R is not --
//             unlike locate's containment rule.
//   run       a maximal stretch of consecutive bases of ONE record whose codes are all in the class, end - begin >= min_len; a record's
//             end always ends a run.  code = the code of the run's first base.  EACH: every code of the class is a class of its own.
//   masked    runs of bases g with an odd number of mask toggles <= g, split at record ends; code 0.  No sequence is decoded.
//   never     bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no run.
//   order     ascending (record, begin); the same bytes on every run and for every piece size.
//
// A run may span millions of bases, so most tiles inside it hold neither of its ends.  In stream order the k-th run START pairs with the
// k-th run END (runs are disjoint and ordered), so the two are found apart and no kernel waits for another:
//   k_runs_mark<false>  a wavefront per tile of 4096 bases, 64 bases a lane as two 16-byte loads (tiles start on an even base, the lanes at
//                       the range's end load byte by byte).  Membership of a lane's 64 bases is a 64-bit mask M made from the four bit
//                       planes (x >> b) & 0x11111111; C = "continues the run of the base in front" = M & (M << 1 | in front) & ~record
//                       starts (EACH: & same code, x ^ (x moved up one nibble)).  Starts = M & ~C, ends = M & ~(C >> 1): two popcounts a
//                       lane, two wave sums a tile, no atomics.  The base in front of a lane's first and behind its last come from the
//                       neighbour lanes, at the tile's two edges from one bounds-checked byte each.
//   scan                the per-tile counts of starts and of ends (scan_exclusive_u64).
//   k_runs_mark<true>   recomputes the tiles that have events and stores the positions (u64) at their ranks from a wave prefix sum.
//   k_runs_pair         a lane per candidate: length, the min_len test as a flag for the next scan, a wave sum of the kept bases.
//   k_runs_rows         a lane per kept run: its record by one upper_bound on rec_base, its code from the piece's bytes, a 32-byte row.
// A run that lies wholly inside one lane and is shorter than min_len is dropped by both mark passes alike (the prefilter): the candidate
// tables of `ACGT` + EACH at min_len 10 are then a few entries per lane instead of one per base.
// The soft mask needs no sweep: the toggle list is first reduced to the positions where the parity really changes (equal toggles cancel in
// pairs: k_runs_tog_keep, a scan, k_runs_tog_pack), then a lane per record counts its stretches (two upper_bounds and the parity at its
// first base), a scan, a lane per stretch clips its interval to its record, and k_runs_pair / k_runs_rows finish as above.
#pragma once

#define RUNS_TILE 4096u
#define RUNS_PIECE_DEFAULT (1ull << 31)      // bases swept per decode (NAF_GPU_RUNS_PIECE)
#define RUNS_FLAGS (NAF_GPU_RUNS_EACH | NAF_GPU_RUNS_MASKED)

// bit 0 of each of a dword's eight nibbles -> eight adjacent bits
__device__ __forceinline__ u32 runs_pack8(u32 y)
{
    y &= NIB_L; y = (y | (y >> 3)) & 0x03030303u; y = (y | (y >> 6)) & 0x000F000Fu;
    return (y | (y >> 12)) & 0xFFu;
}
// bit 0 of every nibble of y whose code is in `set` (the same in every lane: the ANDs are picked by scalar branches)
__device__ __forceinline__ u32 runs_member(u32 y, u32 set)
{
    u32 lo[4], hi[4]; nib_products(y, lo, hi);
    u32 m = 0;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const u32 sub = (set >> (4 * h)) & 15u;
        if (sub) {
            u32 in = 0;
#pragma unroll
            for (int l = 0; l < 4; l++) if ((sub >> l) & 1u) in |= lo[l];
            m |= in & hi[h];
        }
    }
    return m;
}

// WRITE = false: cnt_s[t] / cnt_e[t] = run starts / run ends of tile t.
// WRITE = true:  the starts of tile t at starts[off_s[t] ...] and its ends (exclusive positions) at ends[off_e[t] ...], in position order;
//                a tile without events returns at once.  cap: entries of either table.
// seq: pointer to packed byte 0 of the stream; bytes [p_lo / 2, b_end) of it may be read.  Records [r_lo, r_hi) are swept:
// rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.  set, each, min_len: the same in every lane.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_runs_mark(const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0,
                                                  u32 set, u32 each, u64 min_len, u64 *cnt_s, u64 *cnt_e,
                                                  const u64 *off_s, const u64 *off_e, u64 *starts, u64 *ends, u64 cap)
{
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    if (WRITE) { if (off_s[t] == off_s[t + 1] && off_e[t] == off_e[t + 1]) return; }
    const u64 g = t0 + t * RUNS_TILE + lane * 64;                                 // the lane's first base
    const u64 lo = g > p_lo ? g : p_lo, hi = g + 64 < p_hi ? g + 64 : p_hi;       // the bases of it that are swept
    const bool active = g < p_hi && lo < hi;
    u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (active) packed_load64(seq, b_end, g, x);
    const u32 pc = packed_front(seq, p_lo, g, active, lane, x), nc = packed_behind(seq, b_end, g, active, lane, x);

    u64 S = 0, E = 0;
    if (active) {
        const u32 a = (u32)(lo - g), b = (u32)(hi - g);                           // a: 0 or 1, b: 1 .. 64
        const u64 V = (b == 64 ? ~0ull : (1ull << b) - 1) & ~((1ull << a) - 1);
        u64 M = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) M |= (u64)runs_pack8(runs_member(x[i], set)) << (8 * i);
        M &= V;
        const bool prev_in = g > p_lo && ((set >> pc) & 1u), next_in = g + 64 < p_hi && ((set >> nc) & 1u);
        // record starts at g + j, j = 0 .. 64 (one upper_bound, then linear; empty records share a base and set the same bit again)
        u64 B = 0; bool b64 = false;
        if (M) {
            u64 i = lo == p_lo ? r_lo : upper_bound_u64(rec_base, r_lo, r_hi + 1, lo - 1);     // the first record that starts at or behind lo
            for (; i <= r_hi; i++) {
                const u64 d = rec_base[i] - g;
                if (d > 64) break;
                if (d == 64) b64 = true; else B |= 1ull << d;
            }
        }
        u64 C = M & ((M << 1) | (prev_in ? 1ull : 0ull)) & ~B;                    // base j goes on with the run of base j - 1
        bool c64 = next_in && (M >> 63) && !b64;
        if (each) {
            u64 Q = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const u32 d = x[i] ^ ((x[i] << 4) | (i ? x[(i + 7) & 7] >> 28 : pc));     // every base against the one in front of it
                u32 z = d | (d >> 1); z |= z >> 2;
                Q |= (u64)runs_pack8(~z) << (8 * i);
            }
            C &= Q;
            c64 = c64 && nc == (x[7] >> 28);
        }
        S = M & ~C;
        E = M & ~((C >> 1) | (c64 ? 1ull << 63 : 0ull));
        if (min_len > 1) {                                                        // the prefilter: short runs that lie wholly in this lane
            for (u64 s = S; s; s &= s - 1) {
                const u32 j = (u32)__builtin_ctzll(s);
                const u64 e = E >> j;
                if (!e) break;
                const u32 k = (u32)__builtin_ctzll(e);
                if ((u64)k + 1 < min_len) { S &= ~(1ull << j); E &= ~(1ull << (j + k)); }
            }
        }
    }
    const u32 ns = (u32)__popcll(S), ne = (u32)__popcll(E);
    if (!WRITE) {
        const u32 ts = wave_sum_u32(ns), te = wave_sum_u32(ne);
        if (lane == 0) { cnt_s[t] = ts; cnt_e[t] = te; }
    } else {
        u64 ps = off_s[t] + wave_prefix_u32(ns, lane), pe = off_e[t] + wave_prefix_u32(ne, lane);
        for (u64 s = S; s; s &= s - 1, ps++) if (ps < cap) starts[ps] = g + (u32)__builtin_ctzll(s);
        for (u64 e = E; e; e &= e - 1, pe++) if (pe < cap) ends[pe] = g + (u32)__builtin_ctzll(e) + 1;
    }
}

// a lane per candidate k < n: flag[k] = 1 when the run [starts[k], ends[k]) has min_len bases (flag[n] = 0: the scan's total lands there);
// sum[0] += the kept bases, sum[1] += candidates whose end is not behind their start (there are none)
__global__ __launch_bounds__(256) void k_runs_pair(const u64 *starts, const u64 *ends, u64 n, u64 min_len, u64 *flag, unsigned long long *sum)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    u64 kept = 0; bool bad = false;
    if (k < n) {
        const u64 s = starts[k], e = ends[k];
        bad = e <= s;
        if (!bad && e - s >= min_len) kept = e - s;
    }
    if (k <= n) flag[k] = kept ? 1 : 0;
    kept = wave_sum_u64(kept);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&sum[0], (unsigned long long)kept);
    if (bad) atomicAdd(&sum[1], 1ull);
}
// a lane per candidate: the row of a kept one, at rows[32 (out_base + flag[k])].  flag: the scan of k_runs_pair's.  seq: the piece's packed
// bytes, or null (code 0).  Records [r_lo, r_hi) hold every start.  rows: any alignment.
__global__ __launch_bounds__(256) void k_runs_rows(const u64 *starts, const u64 *ends, const u64 *flag, u64 n, const u64 *rec_base, u64 r_lo, u64 r_hi,
                                                   const u8 *seq, u64 out_base, u8 *rows)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || flag[k + 1] == flag[k]) return;
    const u64 s = starts[k], e = ends[k];
    const u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, s) - 1;               // the last record that starts at or before s (empty ones share a base): the one that has it
    const u64 base = rec_base[r];
    const u32 code = seq ? ((u32)seq[s >> 1] >> (4 * (u32)(s & 1))) & 15u : 0u;
    u8 *o = rows + (out_base + flag[k]) * 32;
    st64(o, r); st64(o + 8, s - base); st64(o + 16, e - base); st32(o + 24, code); st32(o + 28, 0);
}

// keep[i] = 1 for the last toggle of a group of equal ones that has an odd number of members (an even group changes no parity); keep[n] = 0
__global__ __launch_bounds__(256) void k_runs_tog_keep(const u64 *tg, u64 n, u64 *keep)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    u64 v = 0;
    if (i < n && (i + 1 == n || tg[i + 1] != tg[i])) {
        const u64 first = tg[i] ? upper_bound_u64(tg, 0, i, tg[i] - 1) : 0;       // the group's first member
        v = (i - first + 1) & 1;
    }
    keep[i] = v;
}
__global__ __launch_bounds__(256) void k_runs_tog_pack(const u64 *tg, const u64 *keep, u64 n, u64 *out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n && keep[i + 1] != keep[i]) out[keep[i]] = tg[i];
}
// tc: nc strictly increasing toggles; toggle i starts a masked stretch when i is even.  cnt[i] = stretches of record first + i; cnt[n] = 0
__global__ __launch_bounds__(256) void k_runs_mask_count(const u64 *rec_base, u64 first, u64 n, const u64 *tc, u64 nc, u64 *cnt)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    u64 v = 0;
    if (i < n) {
        const u64 a = rec_base[first + i], b = rec_base[first + i + 1];
        if (b > a) {
            const u64 ka = upper_bound_u64(tc, 0, nc, a), kb = upper_bound_u64(tc, ka, nc, b - 1);   // toggles <= a, toggles <= b - 1
            v = (ka & 1) + ((kb + 1) / 2 - (ka + 1) / 2);                         // the one that holds base a, and the even toggles in (a, b - 1]
        }
    }
    cnt[i] = v;
}
// a lane per stretch j < total: row_scan = the scan of the counts; its record, its toggle pair and the interval clipped to the record
__global__ __launch_bounds__(256) void k_runs_mask_cand(const u64 *rec_base, u64 first, u64 n, const u64 *row_scan, const u64 *tc, u64 nc, u64 total, u64 *starts, u64 *ends)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= total) return;
    const u64 ri = upper_bound_u64(row_scan, 0, n + 1, j) - 1;                    // the last record whose stretches start at or before this one: the one that has it
    const u64 a = rec_base[first + ri], b = rec_base[first + ri + 1];
    const u64 ka = upper_bound_u64(tc, 0, nc, a);
    const u64 i = (ka & ~1ull) + 2 * (j - row_scan[ri]);
    const u64 s = tc[i], e = i + 1 < nc ? tc[i + 1] : b;
    starts[j] = s > a ? s : a; ends[j] = e < b ? e : b;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// 0, or NAF_GPU_EARG for what is no class
extern "C" int naf_gpu_parse_base_class(const char *text, uint16_t *set)
{
    if (!text || !set) return NAF_GPU_EARG;
    const bool inv = text[0] == '^';
    const char *p = text + (inv ? 1 : 0);
    if (!*p) return NAF_GPU_EARG;
    u32 s = 0;
    for (; *p; p++) {
        const int k = base_code(*p);
        if (k < 0) return NAF_GPU_EARG;
        s |= 1u << k;
    }
    *set = (uint16_t)(inv ? ~s & 0xFFFFu : s);
    return 0;
}

// what both kinds of call do with a table of candidates: the min_len flags, their scan (*here = the kept ones) and -- when writing -- the rows
// behind the `before` of earlier tables.  A bare NAF_GPU_ECAP when before + *here > run_cap: nothing of this table has then been written.
static int runs_finish(naf_gpu_ctx *c, const u64 *starts, const u64 *ends, u64 n, u64 min_len, const u64 *rec_base, u64 r_lo, u64 r_hi, const u8 *seq,
                       unsigned long long *d_sum, bool writing, u8 *d_runs, u64 run_cap, u64 before, u64 *here)
{
    LAUNCH_LIMIT(c, n + 1, 1, "runs: %llu candidates are too many for one launch: set NAF_GPU_RUNS_PIECE to fewer bases", (unsigned long long)n);
    u64 *flag = arena_new<u64>(c, n + 2);
    if (!flag) return ctx_fail(c, NAF_GPU_ENOMEM, "runs: no room for the flags of %llu candidates: set NAF_GPU_RUNS_PIECE to fewer bases", (unsigned long long)n);
    LAUNCH(c, "unnaf_runs_pair", k_runs_pair, (u32)((n + 256) / 256), 256, 0, starts, ends, n, min_len, flag, d_sum);
    int rc = scan_exclusive_u64(c, flag, n + 1, (u64 *)nullptr); if (rc) return rc;
    if ((rc = ctx_readback(c, here, flag + n, 8))) return rc;
    if (writing && *here) {
        if (before + *here > run_cap) return NAF_GPU_ECAP;
        if (!d_runs) return ctx_fail(c, NAF_GPU_EARG, "runs: no place for the rows (d_runs is NULL)");
        LAUNCH(c, "unnaf_runs_rows", k_runs_rows, (u32)((n + 255) / 256), 256, 0, starts, ends, (const u64 *)flag, n, rec_base, r_lo, r_hi, seq, before, d_runs);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

// write: the rows go to d_runs (run_cap entries); too small a capacity is found before anything is written.
static int runs_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, u32 set, int flags, u64 min_len, u64 first, u64 count, u8 *d_runs, size_t run_cap,
                    u64 *n_runs, u64 *n_bases, bool write)
{
    if (!c || !d_naf || !n_runs) return NAF_GPU_EARG;
    *n_runs = 0;
    if (n_bases) *n_bases = 0;
    const bool masked = (flags & NAF_GPU_RUNS_MASKED) != 0, each = (flags & NAF_GPU_RUNS_EACH) != 0;
    if (flags & ~(int)RUNS_FLAGS) return ctx_fail(c, NAF_GPU_EARG, "runs: flags %d: only bits 0 (NAF_GPU_RUNS_EACH) and 1 (NAF_GPU_RUNS_MASKED) are defined", flags);
    if (masked && (set || each)) return ctx_fail(c, NAF_GPU_EARG, "runs: NAF_GPU_RUNS_MASKED takes no class (set 0x%04X) and no NAF_GPU_RUNS_EACH", set);
    if (!masked && !set) return ctx_fail(c, NAF_GPU_EARG, "runs: the class is empty (set 0)");
    if (!min_len) return ctx_fail(c, NAF_GPU_EARG, "runs: min_len 0: a run has at least one base");
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT | (masked ? FRONT_MASK : 0), "runs", "runs of bases cannot be listed", first, &count, pl);   // the mask only when asked for
    if (rc || !count) return rc;
    const EmitP &P = pl.P;
    const bool tracing = ctx_tracing(c);
    unsigned long long *d_sum = arena_new<unsigned long long>(c, 2); if (!d_sum) return NAF_GPU_ENOMEM;      // [0] the kept bases, [1] candidates that are no interval
    u64 total = 0, cands = 0, sum[2] = { 0, 0 };
    size_t n_pieces = 0; u64 decoded = 0;

    if (masked) {
        HIP_TRY(c, hipMemsetAsync(d_sum, 0, 16, c->stream));
        const u64 nt = P.masking ? P.n_toggles : 0;
        if (nt) {
            LAUNCH_LIMIT(c, std::max(nt, count) + 1, 1, "runs: %llu mask toggles, %llu records: too many for one launch", (unsigned long long)nt, (unsigned long long)count);
            // the toggles that change the parity
            u64 *keep = arena_new<u64>(c, nt + 2); if (!keep) return NAF_GPU_ENOMEM;
            LAUNCH(c, "unnaf_runs_mask_keep", k_runs_tog_keep, (u32)((nt + 256) / 256), 256, 0, P.toggles, nt, keep);
            if ((rc = scan_exclusive_u64(c, keep, nt + 1, (u64 *)nullptr))) return rc;
            u64 nc = 0;
            if ((rc = ctx_readback(c, &nc, keep + nt, 8))) return rc;
            u64 *tc = arena_new<u64>(c, nc + 1), *cnt = arena_new<u64>(c, count + 2); if (!tc || !cnt) return NAF_GPU_ENOMEM;
            LAUNCH(c, "unnaf_runs_mask_pack", k_runs_tog_pack, (u32)((nt + 255) / 256), 256, 0, P.toggles, (const u64 *)keep, nt, tc);
            // the stretches of every record
            LAUNCH(c, "unnaf_runs_mask_count", k_runs_mask_count, (u32)((count + 256) / 256), 256, 0, P.rec_base, first, count, (const u64 *)tc, nc, cnt);
            if ((rc = scan_exclusive_u64(c, cnt, count + 1, (u64 *)nullptr))) return rc;
            if ((rc = ctx_readback(c, &cands, cnt + count, 8))) return rc;
            if (cands) {
                LAUNCH_LIMIT(c, cands, 1, "runs: %llu masked intervals are too many for one launch", (unsigned long long)cands);
                u64 *starts = arena_new<u64>(c, cands), *ends = arena_new<u64>(c, cands);
                if (!starts || !ends) return ctx_fail(c, NAF_GPU_ENOMEM, "runs: no room for %llu masked intervals", (unsigned long long)cands);
                LAUNCH(c, "unnaf_runs_mask_cand", k_runs_mask_cand, (u32)((cands + 255) / 256), 256, 0, P.rec_base, first, count, (const u64 *)cnt, (const u64 *)tc, nc, cands, starts, ends);
                rc = runs_finish(c, starts, ends, cands, min_len, P.rec_base, first, first + count, nullptr, d_sum, write, d_runs, run_cap, 0, &total);
                if (rc == NAF_GPU_ECAP) { *n_runs = total; return cap_fail(c, "runs", "runs", total, run_cap); }
                if (rc) return rc;
            }
        }
    } else {
        std::vector<RecPiece> pieces;
        if ((rc = piece_plan(c, P, first, count, "RUNS_PIECE", RUNS_PIECE_DEFAULT, pieces))) return rc;
        n_pieces = pieces.size();
        PieceSweep sw(c, d_naf, pl, "runs");
        u64 cands_of[2] = { 0, 0 };                                                 // of the counting and of the writing sweep
        rc = count_then_write(sw, pieces, RUNS_TILE, { "runs", write, run_cap, d_sum, 16 }, &total,
                              [&](const RecPiece &pc, const PieceSweep::Tiles &tl, bool writing, u64 before, u64 *here) -> int {
            const u64 ntiles = tl.ntiles;
            u64 *cnt_s = arena_new<u64>(c, ntiles + 2), *cnt_e = arena_new<u64>(c, ntiles + 2);
            if (!cnt_s || !cnt_e) return ctx_fail(c, NAF_GPU_ENOMEM, "runs: no room for the counts of %llu tiles: set NAF_GPU_RUNS_PIECE to fewer bases", (unsigned long long)ntiles);
            HIP_TRY(c, hipMemsetAsync(cnt_s + ntiles, 0, 8, c->stream));
            HIP_TRY(c, hipMemsetAsync(cnt_e + ntiles, 0, 8, c->stream));
#define RUNS_LAUNCH(W, name, st, en, cap) LAUNCH(c, name, k_runs_mark<W>, (u32)ntiles, 64, 0, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, set, each ? 1u : 0u, min_len, \
                                              cnt_s, cnt_e, (const u64 *)cnt_s, (const u64 *)cnt_e, st, en, cap)
            RUNS_LAUNCH(false, "unnaf_runs_count", (u64 *)nullptr, (u64 *)nullptr, (u64)0);
            u64 ns = 0, ne = 0;
            int r = tile_totals(c, ntiles, cnt_s, &ns, cnt_e, &ne); if (r) return r;
            if (ns != ne) return ctx_fail(c, NAF_GPU_EFORMAT, "runs: %llu run starts and %llu run ends in one piece", (unsigned long long)ns, (unsigned long long)ne);
            if (!ns) return 0;
            // (in the worst case one start and one end per two bases of the piece -- per base with NAF_GPU_RUNS_EACH at min_len 1)
            u64 *starts = arena_new<u64>(c, ns), *ends = arena_new<u64>(c, ns);
            if (!starts || !ends) return ctx_fail(c, NAF_GPU_ENOMEM, "runs: no room for %llu run starts and ends of a piece of %llu bases: set NAF_GPU_RUNS_PIECE to fewer bases",
                                                  (unsigned long long)ns, (unsigned long long)(pc.p_hi - pc.p_lo));
            RUNS_LAUNCH(true, "unnaf_runs_write", starts, ends, ns);
#undef RUNS_LAUNCH
            cands_of[writing] += ns;
            return runs_finish(c, starts, ends, ns, min_len, P.rec_base, pc.r_lo, pc.r_hi, tl.seq, d_sum, writing, d_runs, run_cap, before, here);
        });
        *n_runs = total;
        if (rc) return rc;
        cands = cands_of[write];
        decoded = sw.decoded;
    }
    *n_runs = total;
    if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc;
    if (sum[1]) return ctx_fail(c, NAF_GPU_EFORMAT, "runs: %llu run ends do not lie behind their starts", (unsigned long long)sum[1]);
    if (n_bases) *n_bases = sum[0];
    if (tracing) ctx_trace(c, "[runs] runs %llu candidates %llu pieces %zu sequence bytes decoded %llu of %llu mask toggles %llu\n", (unsigned long long)total, (unsigned long long)cands,
                           n_pieces, (unsigned long long)decoded, (unsigned long long)pl.seq_bytes, (unsigned long long)(masked && P.masking ? P.n_toggles : 0));
    return 0;
}

extern "C" int naf_gpu_unnaf_runs_count(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint16_t set, int flags, uint64_t min_len,
                                        uint64_t first, uint64_t count, uint64_t *n_runs, uint64_t *n_bases)
{
    int rc = runs_run(c, (const u8 *)d_naf, naf_len, set, flags, min_len, first, count, nullptr, 0, n_runs, n_bases, false);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_runs(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint16_t set, int flags, uint64_t min_len,
                                  uint64_t first, uint64_t count, naf_gpu_run *d_runs, size_t run_cap, uint64_t *n_runs, uint64_t *n_bases)
{
    int rc = runs_run(c, (const u8 *)d_naf, naf_len, set, flags, min_len, first, count, (u8 *)d_runs, run_cap, n_runs, n_bases, true);
    if (c) arena_settle(c);
    return rc;
}
