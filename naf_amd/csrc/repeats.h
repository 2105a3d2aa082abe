// repeats.h -- perfect tandem repeats of period 1 to 16 per record, listed from the packed 4-bit stream (naf_gpu_unnaf_repeats_count,
// naf_gpu_unnaf_repeats; the two host-only functions, the spec parser and the motif class, are naf_gpu.hip's).  Part of emit.hip (included
// by it, behind translate.h): the front of the call, the pieces, the decode of a piece's bytes and count-then-write are payload.h's; the
// lane's 64 bases are packed.h's; the bit planes and the packing of a dword's nibbles are runs.h's; this file holds the kernels and their
// launches.
//
// The contract (include/naf_gpu.h carries it too):
//   repeat    a maximal interval [begin, end) of bases of ONE record, each stored as exactly A, C, G or T/U, with x[i] == x[i + p] for
//             begin <= i < end - p and end - begin >= 2p; a record's end always ends it.  Two of one period may share up to p - 1 bases.
//   motif     the first p bases, base i at bits 2i, 2i + 1 (A 0, C 1, G 2, T 3).  A motif that is a whole power of a shorter word is no row.
//   filters   copies = (end - begin) / p >= min_copies[p - 1], end - begin >= min_len; WHOLE_UNITS: end = begin + copies p before that test.
//   never     bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no repeat.
//   order     ascending (record, begin, period); the same bytes on every run and for every piece size.
//
// "Base j continues" at period p: C_p[j] = base j is A/C/G/T, equals base j - p, and no record starts in (j - p, j].  The repeat is a run of
// C_p, lengthened by p at the front; a run of millions of bases costs only its two ends, which are found apart as in runs.h and paired by
// rank (within one period the runs are disjoint and ordered).  No kernel waits for another:
//   k_repeats_mark<false>  a wavefront per tile of 4096 bases, 64 bases a lane as two 16-byte loads.  The stream is read ONCE for all
//                          periods; the loop over them is over a scalar bit set.  The lane keeps its eight dwords and the three in front of
//                          them (the previous lane's top ones, three shuffles a tile; lane 0 reads bounds-checked bytes, never below the
//                          piece's first) -- eleven dwords for all sixteen periods.  Per period: Q = nibble equality of the eight dwords
//                          against the eleven moved by p nibbles (one v_alignbit a dword), C = M & Q & ~(record starts smeared over p
//                          positions) -- equality with an A/C/G/T base makes base j - p one too --, and the bit in front, C_p[g - 1], from
//                          the front dwords alone.  Starts = C & ~(C << 1 | in front); ends, exclusive, = ~C & (C << 1 | in front), so no
//                          lane needs the base behind it; the lane that holds the piece's last base closes a run that reaches it.  Counts
//                          per tile and list (np lists of starts, then np of ends) from one DPP wave scan a period, list-major, and ONE
//                          scan gives every tile's place in every list.
//   k_repeats_mark<true>   recomputes the tiles that have events and stores the positions at their ranks from the same wave scan.
//   k_repeats_keep         a lane per candidate: begin = start - p, the thresholds, then the motif's p bases from the piece's bytes and the
//                          primitivity test on its 2p bits against every proper divisor of p; the flag for the next scan.  The kept bases
//                          in registers over a grid-stride loop, reduced a workgroup in front of one atomic.
//   k_repeats_pack         the kept ones side by side: begin, end, motif and period, still list by list.
//   k_repeats_rows         a lane per kept repeat: its rank is its index in its own period's list plus, for each other period, a bound of
//                          (begin, period) in that list -- the contract's order without a sort.  The rows per period are differences of the
//                          flag scan at the lists' heads.
// A run of C_p that lies wholly in one lane and is shorter than max(min_copies p, min_len, 2p) - p is dropped by both mark passes alike.
#pragma once

#define REPEATS_TILE 4096u
#define REPEATS_PIECE_DEFAULT (1ull << 31)   // bases swept per decode (NAF_GPU_REPEATS_PIECE)
#define REPEATS_FLAGS (NAF_GPU_REPEATS_WHOLE_UNITS)
#define REPEATS_ACGT 0x0116u                 // codes 1 T, 2 G, 4 C, 8 A of "-TGKCYSBAWRDMHVN"
// the table of a piece's lists (u64, on the device): [0 .. 2 np] where each list begins in the entries, [RT_PERIOD + i] the period and
// [RT_COPIES + i] the copies of list i < np, [RT_KEPT .. RT_KEPT + np] where the kept ones of each list begin
#define RT_PERIOD 40
#define RT_COPIES 56
#define RT_KEPT 72
#define RT_SIZE 96

struct RepeatSpec { u32 periods, np; u32 copies[16]; u64 need[16]; };   // bit p - 1 of periods; [p - 1]: min_copies, the prefilter's length of a C_p run

// bit 8 i + j: nibble j of dword y[3 + i] equals the nibble p places in front of it; sh = 4 ((24 - p) & 7), K = (24 - p) >> 3
template <int K>
__device__ __forceinline__ u64 repeats_equal(const u32 (&y)[11], u32 sh)
{
    u64 Q = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 d = y[3 + i] ^ __builtin_amdgcn_alignbit(y[K + i + 1], y[K + i], sh);
        u32 z = d | (d >> 1); z |= z >> 2;
        Q |= (u64)runs_pack8(~z) << (8 * i);
    }
    return Q;
}

// WRITE = false: cnt[l ntiles + t] = entries of list l in tile t; list i < np: the run starts of the i-th period asked for, np + i: its ends.
// WRITE = true:  the entries of list l of tile t at ent[off[l ntiles + t] ...], in order; a tile without entries returns at once.
// seq: pointer to packed byte 0 of the stream; bytes [p_lo / 2, b_end) of it may be read.  Records [r_lo, r_hi) are swept:
// rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.  R, cap: the same in every lane.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_repeats_mark(const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0, u64 ntiles,
                                                     RepeatSpec R, u64 *cnt, const u64 *off, u64 *ent, u64 cap)
{
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    if (WRITE) {
        const bool has = lane < 2 * R.np && off[lane * ntiles + t] != off[lane * ntiles + t + 1];
        if (!__ballot(has)) return;
    }
    const u64 g = t0 + t * REPEATS_TILE + lane * 64;                              // the lane's first base
    const u64 lo = g > p_lo ? g : p_lo, hi = g + 64 < p_hi ? g + 64 : p_hi;       // the bases of it that are swept
    const bool active = g < p_hi && lo < hi;
    u32 y[11] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };                              // y[3 ..]: the lane's 64 bases; y[0 .. 2]: the 24 in front
    {
        u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (active) packed_load64(seq, b_end, g, x);
#pragma unroll
        for (int i = 0; i < 8; i++) y[3 + i] = x[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { const u32 up = (u32)__shfl_up((int)y[8 + i], 1); y[i] = lane ? up : 0u; }
    if (active && lane == 0) {                                                    // bytes [(g >> 1) - 12, g >> 1) that do not lie below the piece's first
        const u64 b0 = g >> 1, first = p_lo >> 1;
#pragma unroll
        for (u32 i = 0; i < 12; i++)
            if (b0 + i >= 12 + first) y[i >> 2] |= (u32)seq[b0 + i - 12] << (8 * (i & 3));
    }

    u64 M = 0, V = 0, Bh = 0, Bl = 0;                                             // A/C/G/T; swept; record starts at g + d: bit d of Bh, bit 64 + d of Bl (d < 0)
    u32 b = 0;
    const u32 c1 = y[2] >> 28;                                                    // the code of base g - 1
    const bool front = active && g > p_lo && ((REPEATS_ACGT >> c1) & 1u);
    if (active) {
        const u32 a = (u32)(lo - g); b = (u32)(hi - g);                           // a: 0 or 1, b: 1 .. 64
        V = kmer_bits(a, b);
#pragma unroll
        for (int i = 0; i < 8; i++) M |= (u64)runs_pack8(runs_member(y[3 + i], REPEATS_ACGT)) << (8 * i);
        M &= V;
        if (M || front) {                                                         // one upper_bound, then linear; empty records share a base and set the same bit again
            const u64 w = g > p_lo + 24 ? g - 24 : p_lo;
            for (u64 i = w == p_lo ? r_lo : upper_bound_u64(rec_base, r_lo, r_hi + 1, w - 1); i <= r_hi; i++) {
                const u64 pos = rec_base[i];
                if (pos >= g + 64) break;
                if (pos >= g) Bh |= 1ull << (pos - g); else Bl |= 1ull << (64 - (g - pos));
            }
        }
    }
    const u64 Em = V | (active && hi == p_hi && b < 64 ? 1ull << b : 0ull);       // where an end may lie: the piece's end closes a run
    const u64 f01 = (u64)y[0] | ((u64)y[1] << 32);

    u32 pi = 0;
    for (u32 rest = R.periods; rest; rest &= rest - 1, pi++) {                    // (the same in every lane: a scalar loop)
        const u32 p = (u32)__builtin_ctz(rest) + 1;
        u64 S = 0, E = 0; u32 e64 = 0;
        if (active) {
            const u32 sh = 4 * ((24 - p) & 7);
            const u64 Q = p <= 8 ? repeats_equal<2>(y, sh) : repeats_equal<1>(y, sh);
            u64 kh = Bh, kl = Bl;                                                 // record starts smeared over p positions
            if (kh | kl) {
                u32 w = 1;
                for (; 2 * w <= p; w *= 2) { kh |= (kh << w) | (kl >> (64 - w)); kl |= kl << w; }
                if (p > w) kh |= (kh << (p - w)) | (kl >> (64 - (p - w)));
            }
            const u64 C = M & Q & ~kh;
            bool cin = false;                                                     // C_p[g - 1]
            if (front) {
                const u32 idx = 23 - p, c0 = idx < 16 ? (u32)(f01 >> (4 * idx)) & 15u : (y[2] >> (4 * (idx - 16))) & 15u;
                cin = c0 == c1 && !(Bl >> (64 - p));
            }
            const u64 prev = (C << 1) | (cin ? 1ull : 0ull);
            S = C & ~prev;
            E = ~C & prev & Em;
            e64 = (hi == p_hi && b == 64 && (C >> 63)) ? 1u : 0u;
            const u64 need = R.need[p - 1];
            if (need > 1) {                                                       // the prefilter: short runs that lie wholly in this lane
                for (u64 s = S; s; s &= s - 1) {
                    const u32 j = (u32)__builtin_ctzll(s);
                    if (j == 63) break;
                    const u64 e = E >> (j + 1);
                    if (!e) break;
                    const u32 k = (u32)__builtin_ctzll(e) + 1;
                    if ((u64)k < need) { S &= ~(1ull << j); E &= ~(1ull << (j + k)); }
                }
            }
        }
        const u32 v = (u32)__popcll(S) | (((u32)__popcll(E) + e64) << 16);        // a tile has at most 2112 of either
        const u32 inc = wave_scan_inclusive<u32, OpAdd>(v);
        const u64 ls = (u64)pi * ntiles + t, le = (u64)(R.np + pi) * ntiles + t;
        if (!WRITE) {
            if (lane == 63) { cnt[ls] = inc & 0xFFFFu; cnt[le] = inc >> 16; }
        } else {
            const u32 pre = inc - v;
            u64 ps = off[ls] + (pre & 0xFFFFu), pe = off[le] + (pre >> 16);
            for (u64 s = S; s; s &= s - 1, ps++) if (ps < cap) ent[ps] = g + (u32)__builtin_ctzll(s);
            for (u64 e = E; e; e &= e - 1, pe++) if (pe < cap) ent[pe] = g + (u32)__builtin_ctzll(e);
            if (e64 && pe < cap) ent[pe] = g + 64;
        }
    }
}

// T[l] = off[l ntiles], l <= 2 np; the period and the copies of every list
__global__ __launch_bounds__(64) void k_repeats_heads(const u64 *off, u64 ntiles, RepeatSpec R, u64 *T)
{
    const u32 l = threadIdx.x;
    if (l <= 2 * R.np) T[l] = off[(u64)l * ntiles];
    if (l == 0) {
        u32 pi = 0;
        for (u32 rest = R.periods; rest; rest &= rest - 1, pi++) { const u32 p = (u32)__builtin_ctz(rest) + 1; T[RT_PERIOD + pi] = p; T[RT_COPIES + pi] = R.copies[p - 1]; }
    }
}
// T[RT_KEPT + i] = flag[T[i]], i <= np: where the kept ones of each list begin (flag: the scan of k_repeats_keep's)
__global__ __launch_bounds__(64) void k_repeats_kept(const u64 *flag, u32 np, u64 *T) { if (threadIdx.x <= np) T[RT_KEPT + threadIdx.x] = flag[T[threadIdx.x]]; }

struct RepeatAt { u64 begin, end; u32 motif, p, pi; };
// base i of [begin, begin + p) at bits 2i, 2i + 1: A 0, C 1, G 2, T 3 (the bases of a repeat are these four)
__device__ __forceinline__ u32 repeats_motif(const u8 *seq, u64 begin, u32 p)
{
    u32 m = 0;
    for (u32 i = 0; i < p; i++) {
        const u64 q = begin + i;
        const u32 code = ((u32)seq[q >> 1] >> (4 * (u32)(q & 1))) & 15u;
        m |= (code == 8 ? 0u : code == 4 ? 1u : code == 2 ? 2u : 3u) << (2 * i);
    }
    return m;
}
// a motif of p bases that is no whole power of a shorter word
__device__ __forceinline__ bool repeats_primitive(u32 m, u32 p)
{
    for (u32 d = 1; 2 * d <= p; d++)
        if (p % d == 0 && (m >> (2 * d)) == (m & ((1u << (2 * (p - d))) - 1))) return false;
    return true;
}
// The repeat of candidate k < n = T[np] (its start ent[k], its end ent[n + k]); false: one that the call does not keep.  *bad: no interval.
__device__ __forceinline__ bool repeats_at(const u64 *ent, const u64 *T, u32 np, u64 k, const u8 *seq, u64 min_len, u32 whole, RepeatAt &o, bool *bad)
{
    u32 pi = 0;
    while (pi + 1 < np && k >= T[pi + 1]) pi++;
    const u64 n = T[np], s = ent[k], e = ent[n + k];
    const u32 p = (u32)T[RT_PERIOD + pi];
    *bad = e <= s;
    if (*bad) return false;
    o.begin = s - p; o.pi = pi; o.p = p;
    const u64 copies = (e - o.begin) / p;
    o.end = whole ? o.begin + copies * p : e;
    if (copies < T[RT_COPIES + pi] || o.end - o.begin < min_len) return false;
    o.motif = repeats_motif(seq, o.begin, p);
    return repeats_primitive(o.motif, p);
}

// a lane per candidate k < n (grid-stride, at most 2048 workgroups): flag[k] = 1 for a kept one (flag[n] = 0: the scan's total lands there);
// sum[0] += the kept bases, sum[1] += candidates whose end is not behind their start (there are none)
__global__ __launch_bounds__(256) void k_repeats_keep(const u64 *ent, const u64 *T, u32 np, u64 n, const u8 *seq, u64 min_len, u32 whole, u64 *flag, unsigned long long *sum)
{
    __shared__ u64 part[2][4];
    u64 acc[2] = { 0, 0 };
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k <= n; k += (u64)gridDim.x * 256) {
        bool kept = false;
        if (k < n) {
            RepeatAt o; bool bad;
            kept = repeats_at(ent, T, np, k, seq, min_len, whole, o, &bad);
            if (kept) acc[0] += o.end - o.begin;
            acc[1] += bad ? 1 : 0;
        }
        flag[k] = kept ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const u64 v = wave_sum_u64(acc[q]);
        if ((threadIdx.x & 63) == 0) part[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u64 v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (v) atomicAdd(&sum[threadIdx.x], (unsigned long long)v);
    }
}
// a lane per candidate: a kept one, recomputed, at place flag[k] of the three tables; meta = motif | period << 32 | list << 40
__global__ __launch_bounds__(256) void k_repeats_pack(const u64 *ent, const u64 *T, u32 np, u64 n, const u8 *seq, u64 min_len, u32 whole, const u64 *flag, u64 *cb, u64 *ce, u64 *cm)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || flag[k + 1] == flag[k]) return;
    RepeatAt o; bool bad;
    if (!repeats_at(ent, T, np, k, seq, min_len, whole, o, &bad)) return;         // (it was kept: it is one)
    const u64 q = flag[k];
    cb[q] = o.begin; ce[q] = o.end; cm[q] = (u64)o.motif | ((u64)o.p << 32) | ((u64)o.pi << 40);
}
// a lane per kept repeat q < nk: its row at rows[32 (out_base + rank)], rank = its place among the kept of all lists in (begin, period)
// order.  The kept of list i are [T[RT_KEPT + i], T[RT_KEPT + i + 1]) of the tables, ascending in begin.  Records [r_lo, r_hi) hold every
// one.  rows: any alignment.
__global__ __launch_bounds__(256) void k_repeats_rows(const u64 *cb, const u64 *ce, const u64 *cm, u64 nk, const u64 *T, u32 np, const u64 *rec_base, u64 r_lo, u64 r_hi,
                                                      u64 out_base, u8 *rows)
{
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= nk) return;
    const u64 ob = cb[q], oe = ce[q], m = cm[q];
    const u32 pi = (u32)(m >> 40);
    u64 rank = 0;
    for (u32 l = 0; l < np; l++) {
        const u64 a = T[RT_KEPT + l], b = T[RT_KEPT + l + 1];
        if (l == pi) rank += q - a;
        else if (l < pi) rank += upper_bound_u64(cb, a, b, ob) - a;               // a shorter period that begins on the same base goes first
        else rank += (ob ? upper_bound_u64(cb, a, b, ob - 1) : a) - a;
    }
    const u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, ob) - 1;              // the last record that starts at or before ob (empty ones share a base): the one that has it
    const u64 base = rec_base[r];
    u8 *o = rows + (out_base + rank) * 32;
    st64(o, r); st64(o + 8, ob - base); st64(o + 16, oe - base); st32(o + 24, (u32)m); st32(o + 28, (u32)(m >> 32) & 0xFFu);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// write: the rows go to d_rows (row_cap entries); too small a capacity is found before anything is written.
static int repeats_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, const naf_gpu_repeat_spec *spec, int flags, u64 min_len, u64 first, u64 count,
                       u8 *d_rows, size_t row_cap, u64 *n_repeats, u64 *n_bases, u64 *per_period, bool write)
{
    if (!c || !d_naf || !n_repeats) return NAF_GPU_EARG;
    *n_repeats = 0;
    if (n_bases) *n_bases = 0;
    if (per_period) memset(per_period, 0, 16 * sizeof *per_period);
    if (!spec) return ctx_fail(c, NAF_GPU_EARG, "repeats: no spec (NULL)");
    if (flags & ~(int)REPEATS_FLAGS) return ctx_fail(c, NAF_GPU_EARG, "repeats: flags %d: only bit 0 (NAF_GPU_REPEATS_WHOLE_UNITS) is defined", flags);
    if (!min_len) return ctx_fail(c, NAF_GPU_EARG, "repeats: min_len 0: a repeat has at least two bases");
    RepeatSpec R; memset(&R, 0, sizeof R);
    for (u32 p = 1; p <= 16; p++) {
        const u32 mc = spec->min_copies[p - 1];
        if (mc == 1) return ctx_fail(c, NAF_GPU_EARG, "repeats: min_copies[%u] is 1: a repeat of period %u has at least 2 copies (0: the period is not searched)", p - 1, p);
        if (!mc) continue;
        R.periods |= 1u << (p - 1); R.np++; R.copies[p - 1] = mc;
        R.need[p - 1] = std::max<u64>((u64)mc * p, min_len) - p;
    }
    if (!R.np) return ctx_fail(c, NAF_GPU_EARG, "repeats: the spec searches no period (every min_copies is 0)");
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, "repeats", "tandem repeats cannot be listed", first, &count, pl);
    if (rc || !count) return rc;
    const EmitP &P = pl.P;
    const bool tracing = ctx_tracing(c);
    const u32 np = R.np, whole = (flags & NAF_GPU_REPEATS_WHOLE_UNITS) ? 1u : 0u;
    unsigned long long *d_sum = arena_new<unsigned long long>(c, 2); if (!d_sum) return NAF_GPU_ENOMEM;      // [0] the kept bases, [1] candidates that are no interval
    u64 total = 0, sum[2] = { 0, 0 };
    u64 cands_of[2] = { 0, 0 }, per_of[2][16];                                    // of the counting and of the writing sweep
    memset(per_of, 0, sizeof per_of);

    std::vector<RecPiece> pieces;
    if ((rc = piece_plan(c, P, first, count, "REPEATS_PIECE", REPEATS_PIECE_DEFAULT, pieces))) return rc;
    PieceSweep sw(c, d_naf, pl, "repeats");
    rc = count_then_write(sw, pieces, REPEATS_TILE, { "repeats", write, row_cap, d_sum, sizeof sum }, &total,
                          [&](const RecPiece &pc, const PieceSweep::Tiles &tl, bool writing, u64 before, u64 *here) -> int {
        const u64 ntiles = tl.ntiles, nl = 2ull * np * ntiles;
        u64 *cnt = arena_new<u64>(c, nl + 2), *T = arena_new<u64>(c, RT_SIZE);
        if (!cnt || !T) return ctx_fail(c, NAF_GPU_ENOMEM, "repeats: no room for the counts of %llu tiles and %u periods: set NAF_GPU_REPEATS_PIECE to fewer bases", (unsigned long long)ntiles, np);
        HIP_TRY(c, hipMemsetAsync(cnt + nl, 0, 8, c->stream));
#define REPEATS_MARK(W, name, en, cap) LAUNCH(c, name, k_repeats_mark<W>, (u32)ntiles, 64, 0, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, ntiles, \
                                              R, cnt, (const u64 *)cnt, en, cap)
        REPEATS_MARK(false, "unnaf_repeats_count", (u64 *)nullptr, (u64)0);
        int r = scan_exclusive_u64(c, cnt, nl + 1, (u64 *)nullptr); if (r) return r;
        LAUNCH(c, "unnaf_repeats_heads", k_repeats_heads, 1, 64, 0, (const u64 *)cnt, ntiles, R, T);
        u64 head[33];
        if ((r = ctx_readback(c, head, T, (2 * np + 1) * 8))) return r;
        const u64 n = head[np], all = head[2 * np];
        for (u32 i = 0; i <= np; i++)
            if (head[np + i] - n != head[i]) return ctx_fail(c, NAF_GPU_EFORMAT, "repeats: the run starts and the run ends of a period differ in number in one piece");
        if (!n) return 0;
        LAUNCH_LIMIT(c, n + 1, 1, "repeats: %llu candidates are too many for one launch: set NAF_GPU_REPEATS_PIECE to fewer bases", (unsigned long long)n);
        // (at the worst, period 1 at 2 copies and min_len 1 in a text of pairs, a start and an end per two bases)
        u64 *ent = arena_new<u64>(c, all), *flag = arena_new<u64>(c, n + 2);
        if (!ent || !flag) return ctx_fail(c, NAF_GPU_ENOMEM, "repeats: no room for the candidate tables (%llu run starts and ends) of a piece of %llu bases: set NAF_GPU_REPEATS_PIECE to fewer bases",
                                            (unsigned long long)all, (unsigned long long)(pc.p_hi - pc.p_lo));
        REPEATS_MARK(true, "unnaf_repeats_write", ent, all);
#undef REPEATS_MARK
        cands_of[writing] += n;
        LAUNCH(c, "unnaf_repeats_keep", k_repeats_keep, (u32)std::min<u64>((n + 256) / 256, 2048), 256, 0, (const u64 *)ent, (const u64 *)T, np, n, tl.seq, min_len, whole, flag, d_sum);
        if ((r = scan_exclusive_u64(c, flag, n + 1, (u64 *)nullptr))) return r;
        LAUNCH(c, "unnaf_repeats_kept", k_repeats_kept, 1, 64, 0, (const u64 *)flag, np, T);
        u64 kept[17];
        if ((r = ctx_readback(c, kept, T + RT_KEPT, (np + 1) * 8))) return r;
        *here = kept[np];
        { u32 pi = 0; for (u32 rest = R.periods; rest; rest &= rest - 1, pi++) per_of[writing][__builtin_ctz(rest)] += kept[pi + 1] - kept[pi]; }
        if (!writing || !*here) return 0;
        if (before + *here > row_cap) return NAF_GPU_ECAP;
        if (!d_rows) return ctx_fail(c, NAF_GPU_EARG, "repeats: no place for the rows (d_rows is NULL)");
        const u64 nk = *here;
        u64 *tab = arena_new<u64>(c, 3 * nk);
        if (!tab) return ctx_fail(c, NAF_GPU_ENOMEM, "repeats: no room for %llu repeats of a piece: set NAF_GPU_REPEATS_PIECE to fewer bases", (unsigned long long)nk);
        LAUNCH(c, "unnaf_repeats_pack", k_repeats_pack, (u32)((n + 255) / 256), 256, 0, (const u64 *)ent, (const u64 *)T, np, n, tl.seq, min_len, whole, (const u64 *)flag, tab, tab + nk, tab + 2 * nk);
        LAUNCH(c, "unnaf_repeats_rows", k_repeats_rows, (u32)((nk + 255) / 256), 256, 0, (const u64 *)tab, (const u64 *)(tab + nk), (const u64 *)(tab + 2 * nk), nk, (const u64 *)T, np,
               P.rec_base, pc.r_lo, pc.r_hi, before, d_rows);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return 0;
    });
    *n_repeats = total;
    if (rc) return rc;
    if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc;
    if (sum[1]) return ctx_fail(c, NAF_GPU_EFORMAT, "repeats: %llu run ends do not lie behind their starts", (unsigned long long)sum[1]);
    if (n_bases) *n_bases = sum[0];
    if (per_period) memcpy(per_period, per_of[write], 16 * sizeof *per_period);
    if (tracing) ctx_trace(c, "[repeats] rows %llu candidates %llu periods %u pieces %zu sequence bytes decoded %llu of %llu\n", (unsigned long long)total, (unsigned long long)cands_of[write],
                           np, pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes);
    return 0;
}

extern "C" int naf_gpu_unnaf_repeats_count(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_repeat_spec *spec, int flags, uint64_t min_len,
                                           uint64_t first, uint64_t count, uint64_t *n_repeats, uint64_t *n_bases, uint64_t per_period[16])
{
    int rc = repeats_run(c, (const u8 *)d_naf, naf_len, spec, flags, min_len, first, count, nullptr, 0, n_repeats, n_bases, (u64 *)per_period, false);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_repeats(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, const naf_gpu_repeat_spec *spec, int flags, uint64_t min_len,
                                     uint64_t first, uint64_t count, naf_gpu_repeat *d_rows, size_t row_cap, uint64_t *n_repeats, uint64_t *n_bases, uint64_t per_period[16])
{
    int rc = repeats_run(c, (const u8 *)d_naf, naf_len, spec, flags, min_len, first, count, (u8 *)d_rows, row_cap, n_repeats, n_bases, (u64 *)per_period, true);
    if (c) arena_settle(c);
    return rc;
}
