// kmers.h -- exact dense counts of all 4^K k-mers, K = 1 .. 12, per record or per selection, counted in the packed 4-bit stream
// (naf_gpu_kmer_index, naf_gpu_kmer_text, naf_gpu_unnaf_kmers_rows, naf_gpu_unnaf_kmers).  Part of emit.hip (included by it, behind runs.h):
// the front of the call, the pieces and the decode of a piece's bytes are payload.h's (records_front, piece_plan, PieceSweep); the lane's 64
// bases and the twelve behind them are packed.h's; this file holds the index arithmetic, the kernels and their launches.
//
// The contract (include/naf_gpu.h carries it too):
//   index     A = 0, C = 1, G = 2, T/U = 3, two bits a base, the FIRST base the most significant: ascending index = lexicographic order.
//   counted   position g of record r, when bases g .. g + K - 1 all lie in r and each is stored as exactly A, C, G or T/U (codes 8, 4, 2, 1).
//             Any other code invalidates every k-mer that covers it; case plays no part (the mask is not decoded); every start counts.
//   never     bases behind the last record of a malformed archive and the padding nibble of an odd stream are in no k-mer.
//   CANONICAL a counted k-mer adds to min(index, index of its reverse complement); a palindrome counts once per occurrence.
//   PER_RECORD one table of 4^K u64 per record of [first, first + count), and one 40-byte row (record, 0, len, positions, counted) each;
//             without it one table for the selection.  Integer adds: the same bytes on every run and for every piece size.
//
// k_kmer_count: a wavefront per tile of 4096 bases, 64 bases a lane (packed_load64; tiles start on an even base), a workgroup of ONE
// wavefront per contiguous chunk of tiles.  Nothing is expanded to letters.  Per dword the four planes (x >> b) & 0x11111111 give "exactly
// one plane set" (the sum of the planes is 1) and the two index bits of a base, plane1 | plane0 (G or T) and plane2 | plane0 (C or T); each
// is packed as runs.h packs its flags, so a lane holds V, H and L as three 64-bit masks plus twelve bits each for the bases behind its last
// (the neighbour lane's first two dwords by __shfl_down; behind the tile's last lane six bounds-checked bytes).  "Position j is counted" is
// V eroded by K (log2 K shift-and-AND steps over the 76 bits), cut to [p_lo, p_hi) and cut K - 1 in front of every record end that lies in
// or just behind the lane (one upper_bound_u64 on rec_base, then linear).  H and L are interleaved ONCE a lane to M (base j at bits 2 j) and
// R = M with the order of its 2-bit groups reversed: the index of position j is a 2 K-bit window of R, the index of its reverse
// complement the same window of ~M -- no second pass.  The kernel then walks the set bits only.
//   LDS bins     K <= the LDS limit and all of the tile's counted positions in one row: ds_add_u32 into 4^K bins the workgroup keeps across
//                its chunk, flushed (one 64-bit global atomic per non-zero bin, consecutive lanes on consecutive bins) when the row changes
//                and at the chunk's end.  K <= 3: every lane has a copy of the bins of its own (bin b of lane l at word 64 b + l: its own
//                bank), summed at the flush.  A tile adds at most 4096 to a bin and a chunk has at most 256 tiles: no bin reaches 2^32.
//                The limit is 7 (64 KiB of bins, two workgroups a CU): measured 16 times faster than the global atomics at K = 7.
//   global       every other tile: one 64-bit global atomic per counted position into its row's table; the record of a position comes from
//                the walk over the lane's record ends.
// The per-row sum `counted` is accumulated beside the bins: a wave sum in front of one atomic (LDS path: once a flush; global path: the
// lanes of the tile's first two rows summed as k_comp_count sums its rows).  k_kmer_rows, a lane per record, writes the rows and sums
// `positions` (from the lengths alone) and `counted` for h_total: a workgroup reduction in front of the atomic, at most 2048 workgroups.
#pragma once

#define KMER_TILE 4096u
#define KMER_MAX_K 12u
#define KMER_PIECE_DEFAULT (1ull << 31)      // bases swept per decode (NAF_GPU_KMERS_PIECE)
#define KMER_LDS_K_DEFAULT 7u                // the largest K counted in LDS bins (NAF_GPU_KMERS_LDS_K: 0 .. 7)
#define KMER_FLAGS (NAF_GPU_KMER_CANONICAL | NAF_GPU_KMER_PER_RECORD)
#define KMER_NONE (~0ull)

// ---- the bits of a lane ------------------------------------------------------------------------------------------------------------
// of a dword's eight bases, eight bits each: v = stored as exactly A, C, G or T; h, l = the two index bits (meaningful where v is set)
__device__ __forceinline__ void kmer_planes(u32 y, u32 &v, u32 &h, u32 &l)
{
    const u32 p0 = y & NIB_L, p1 = (y >> 1) & NIB_L, p2 = (y >> 2) & NIB_L, p3 = (y >> 3) & NIB_L;
    u32 z = (p0 + p1 + p2 + p3) ^ NIB_L;                                          // a nibble that is not 0: not exactly one plane
    z |= z >> 1; z |= z >> 2;
    v = runs_pack8(~z); h = runs_pack8(p1 | p0); l = runs_pack8(p2 | p0);
}
// bit j, j < 64: bits j .. j + k - 1 of the 76 bits (hi : lo) are all set; k = 1 .. 12, hi has twelve bits
__device__ __forceinline__ u64 kmer_erode(u64 lo, u32 hi32, u32 k)
{
    u64 hi = hi32;
    for (u32 w = 1; w < k; ) {
        const u32 s = w < k - w ? w : k - w;                                      // 1 .. 8
        lo &= (lo >> s) | (hi << (64 - s)); hi &= hi >> s; w += s;
    }
    return lo;
}
// bit i of a -> bit 2 i
__device__ __forceinline__ u64 kmer_spread(u32 a)
{
    u64 x = a;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull; x = (x | (x << 8)) & 0x00FF00FF00FF00FFull; x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull; x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// the 32 two-bit groups of m in reverse order (a bit reversal that stops at the pairs)
__device__ __forceinline__ u64 kmer_reverse_pairs(u64 m)
{
    m = ((m >> 32) | (m << 32));
    m = ((m & 0xFFFF0000FFFF0000ull) >> 16) | ((m & 0x0000FFFF0000FFFFull) << 16);
    m = ((m & 0xFF00FF00FF00FF00ull) >> 8) | ((m & 0x00FF00FF00FF00FFull) << 8);
    m = ((m & 0xF0F0F0F0F0F0F0F0ull) >> 4) | ((m & 0x0F0F0F0F0F0F0F0Full) << 4);
    return ((m & 0xCCCCCCCCCCCCCCCCull) >> 2) | ((m & 0x3333333333333333ull) << 2);
}
// bits [s, s + 24) of the 192 bits (w2 : w1 : w0) under mask; s < 192
__device__ __forceinline__ u32 kmer_window(u64 w0, u64 w1, u64 w2, u32 s, u32 mask)
{
    const u32 q = s >> 6, b = s & 63u;
    const u64 lo = q == 0 ? w0 : q == 1 ? w1 : w2, hi = q == 0 ? w1 : q == 1 ? w2 : 0ull;
    return (u32)((lo >> b) | ((hi << 1) << (63u - b))) & mask;
}
// What a lane knows of its 64 bases and the twelve behind them.  m: base j's two bits at bits 2 j (l) and 2 j + 1 (h) of (m2 : m1 : m0);
// r: the same 96 groups in reverse order, base j at group 95 - j.
struct KmerLane { u64 v; u32 ve; u64 m0, m1, m2, r0, r1, r2; };
// x: the lane's 64 bases; behind: the twelve behind them (48 bits)
__device__ __forceinline__ void kmer_lane(const u32 (&x)[8], u64 behind, KmerLane &k)
{
    u64 v = 0, h = 0, l = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { u32 a, b, c; kmer_planes(x[i], a, b, c); v |= (u64)a << (8 * i); h |= (u64)b << (8 * i); l |= (u64)c << (8 * i); }
    u32 a0, b0, c0, a1, b1, c1;
    kmer_planes((u32)behind, a0, b0, c0); kmer_planes((u32)(behind >> 32) & 0xFFFFu, a1, b1, c1);
    const u32 he = b0 | ((b1 & 15u) << 8), le = c0 | ((c1 & 15u) << 8);
    k.v = v; k.ve = a0 | ((a1 & 15u) << 8);
    k.m0 = (kmer_spread((u32)h) << 1) | kmer_spread((u32)l); k.m1 = (kmer_spread((u32)(h >> 32)) << 1) | kmer_spread((u32)(l >> 32));
    k.m2 = (kmer_spread(he) << 1) | kmer_spread(le);
    k.r0 = kmer_reverse_pairs(k.m2); k.r1 = kmer_reverse_pairs(k.m1); k.r2 = kmer_reverse_pairs(k.m0);
}
// the index of the k-mer at position j of the lane (all of its bases single nucleotides); mask = 4^K - 1
__device__ __forceinline__ u32 kmer_index_at(const KmerLane &k, u32 j, u32 K, u32 mask, bool canon)
{
    const u32 f = kmer_window(k.r0, k.r1, k.r2, 2u * (96u - j - K), mask);
    if (!canon) return f;
    const u32 rc = kmer_window(~k.m0, ~k.m1, ~k.m2, 2u * j, mask);
    return f < rc ? f : rc;
}
// bits [from, to) of a 64-bit mask, from < to <= 64
__device__ __forceinline__ u64 kmer_bits(u32 from, u32 to) { return (to == 64 ? ~0ull : (1ull << to) - 1) & ~((1ull << from) - 1); }
// ---- end of the bits of a lane -----------------------------------------------------------------------------------------------------

// What the workgroup's bins hold goes to `table` (its row's 4^K counters) and the bins are zero again; *counted += the wave's sum of acc.
__device__ __forceinline__ void kmer_flush(u32 *bins, u32 K, u32 lane, unsigned long long *table, unsigned long long *counted, u32 acc)
{
    __syncthreads();
    const u32 nk = 1u << (2 * K);
    if (K <= 3) {                                                                 // lane b sums bin b's 64 copies, each lane starting at a bank of its own
        if (lane < nk) {
            u32 v = 0;
            for (u32 j = 0; j < 64; j++) { u32 *q = &bins[lane * 64 + ((j + lane) & 63u)]; v += *q; *q = 0; }
            if (v) atomicAdd(&table[lane], (unsigned long long)v);
        }
    } else {
        for (u32 b = lane; b < nk; b += 64) {
            const u32 v = bins[b];
            if (v) { atomicAdd(&table[b], (unsigned long long)v); bins[b] = 0; }
        }
    }
    const u32 n = wave_sum_u32(acc);
    if (lane == 0 && n) atomicAdd(counted, (unsigned long long)n);
    __syncthreads();
}

// seq: pointer to packed byte 0 of the stream; bytes [p_lo / 2, b_end) of it may be read.  Records [r_lo, r_hi) are swept: rec_base[r_lo] = p_lo,
// rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo; workgroup c takes tiles [c chunk, (c + 1) chunk) below ntiles, chunk <= 256.
// K, canon, per_record, lds_on: the same in every lane.  counts: table 0 (4^K u64 a row, 8-byte aligned, zeroed by the caller); row = record -
// first with per_record, else 0.  counted[row]: the row's sum.  lds_on: the launch has 4^K words of dynamic LDS (64 x 4^K for K <= 3).
// paths (may be null): tiles counted in LDS bins / by global atomics.
__global__ __launch_bounds__(64) void k_kmer_count(const u8 *seq, u64 b_end, const u64 *rec_base, u64 first, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0,
                                                   u64 ntiles, u32 chunk, u32 K, u32 canon, u32 per_record, u32 lds_on,
                                                   unsigned long long *counts, unsigned long long *counted, unsigned long long *paths)
{
    extern __shared__ u32 kmer_bins[];
    const u32 lane = threadIdx.x;
    const u32 mask = (1u << (2 * K)) - 1u;
    const u64 nk = 1ull << (2 * K);
    const bool own = K <= 3;                                                      // a copy of the bins per lane
    if (lds_on) {
        const u32 entries = (u32)nk * (own ? 64u : 1u);
        for (u32 e = lane; e < entries; e += 64) kmer_bins[e] = 0;
        __syncthreads();
    }
    u64 cur = KMER_NONE; u32 acc = 0;                                             // the row the bins hold, and this lane's part of its sum
    const u64 tb = (u64)xcd_block() * chunk, te = tb + chunk < ntiles ? tb + chunk : ntiles;
    for (u64 t = tb; t < te; t++) {
        const u64 g = t0 + t * KMER_TILE + lane * 64;                             // the lane's first base
        const u64 lo = g > p_lo ? g : p_lo, hi = g + 64 < p_hi ? g + 64 : p_hi;   // the bases of it that are swept
        const bool active = g < p_hi && lo < hi;
        u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (active) packed_load64(seq, b_end, g, x);
        const u64 behind = packed_behind12(seq, b_end, g, active, lane, x);

        KmerLane kl;
        u64 P = 0, rf = 0, rl = 0;                                                // the counted positions; the records of the first and of the last of them
        if (active) {
            kmer_lane(x, behind, kl);
            P = kmer_erode(kl.v, kl.ve, K) & kmer_bits((u32)(lo - g), (u32)(hi - g));
            if (P) {
                const u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, lo) - 1;  // rec_base[r] <= lo < rec_base[r + 1]
                for (u64 i = r + 1; i <= r_hi; i++) {                             // no k-mer over a record's end: K - 1 positions in front of it
                    const u64 d = rec_base[i] - g;                                // >= 1
                    if (d >= 64 + K - 1) break;
                    const u32 from = d > K - 1 ? (u32)d - (K - 1) : 0u, to = d < 64 ? (u32)d : 64u;
                    if (from < to) P &= ~kmer_bits(from, to);
                }
                if (P && per_record) {
                    const u64 jf = (u64)__builtin_ctzll(P), jl = 63u - (u64)__builtin_clzll(P);
                    rf = r; while (rec_base[rf + 1] - g <= jf) rf++;              // (g + jf < p_hi = rec_base[r_hi]: it ends)
                    rl = rf; while (rec_base[rl + 1] - g <= jl) rl++;
                }
            }
        }
        const u64 any = __ballot(P != 0);
        if (!any) continue;
        u64 row = 0; bool single = true;
        if (per_record) {
            row = shfl_u64(rf, __ffsll((long long)any) - 1) - first;
            single = __ballot(P != 0 && (rf - first != row || rl - first != row)) == 0;
        }
        const bool use_lds = lds_on && single;
        if (paths && lane == 0) atomicAdd(&paths[use_lds ? 0 : 1], 1ull);

        if (use_lds) {
            if (row != cur) {
                if (cur != KMER_NONE) { kmer_flush(kmer_bins, K, lane, counts + cur * nk, counted + cur, acc); acc = 0; }
                cur = row;
            }
            acc += (u32)__popcll(P);
            u32 *my = kmer_bins + (own ? lane : 0u);
            const u32 sh = own ? 6u : 0u;
            for (u64 p = P; p; p &= p - 1) atomicAdd(&my[kmer_index_at(kl, (u32)__builtin_ctzll(p), K, mask, canon != 0) << sh], 1u);
        } else {
            u64 rc = per_record ? rf : first;                                     // the record of the position the walk is at
            u64 nb = per_record && P ? rec_base[rc + 1] - g : ~0ull;              // where the next one starts
            u32 run = 0;                                                          // counted positions of rc so far
            for (u64 p = P; p; p &= p - 1) {
                const u32 j = (u32)__builtin_ctzll(p);
                if (j >= nb) {
                    if (run) atomicAdd(&counted[rc - first], (unsigned long long)run);
                    run = 0;
                    do { rc++; nb = rec_base[rc + 1] - g; } while (j >= nb);
                }
                atomicAdd(&counts[(rc - first) * nk + kmer_index_at(kl, j, K, mask, canon != 0)], 1ull);
                run++;
            }
            // the sums of the rows: lanes of one row are summed across the wave and ONE lane adds -- two rounds, then every lane its own
            bool pending = run != 0; const u64 myrow = rc - first;
#pragma unroll 1
            for (int it = 0; it < 2; it++) {
                const u64 pend = __ballot(pending);
                if (!pend) break;
                const int leader = __ffsll((long long)pend) - 1;
                const u64 lrow = shfl_u64(myrow, leader);
                const bool in = pending && myrow == lrow;
                const u32 v = wave_sum_u32(in ? run : 0u);
                if ((int)lane == leader) atomicAdd(&counted[lrow], (unsigned long long)v);
                pending = pending && !in;
            }
            if (pending) atomicAdd(&counted[myrow], (unsigned long long)run);
        }
    }
    if (cur != KMER_NONE) kmer_flush(kmer_bins, K, lane, counts + cur * nk, counted + cur, acc);
}

// A lane per record first + i, i < n (grid-stride): its row at rows + 40 i (any alignment; null: no rows) -- record, 0, len, positions =
// max(len - K + 1, 0), counted[i] (null: 0) --; tot[0] += the positions, tot[1] += the counted, one atomic each a workgroup.
__global__ __launch_bounds__(256) void k_kmer_rows(const u64 *rec_base, u64 first, u64 n, u32 K, const u64 *counted, u8 *rows, unsigned long long *tot)
{
    __shared__ u64 part[2][4];
    u64 sp = 0, sc = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 len = rec_base[first + i + 1] - rec_base[first + i], pos = len >= K ? len - K + 1 : 0, cnt = counted ? counted[i] : 0;
        if (rows) { u8 *o = rows + 40 * i; st64(o, first + i); st64(o + 8, 0); st64(o + 16, len); st64(o + 24, pos); st64(o + 32, cnt); }
        sp += pos; sc += cnt;
    }
    sp = wave_sum_u64(sp); sc = wave_sum_u64(sc);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sp; part[1][threadIdx.x >> 6] = sc; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u64 v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (v) atomicAdd(&tot[threadIdx.x], (unsigned long long)v);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static int kmer_base2(char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    }
    return -1;
}
// 0, or NAF_GPU_EARG for anything but 1 .. 12 letters of ACGTU
extern "C" int naf_gpu_kmer_index(const char *kmer, int canonical, unsigned *k, uint64_t *index)
{
    if (!kmer || !k || !index) return NAF_GPU_EARG;
    const size_t n = strnlen(kmer, KMER_MAX_K + 1);
    if (n < 1 || n > KMER_MAX_K) return NAF_GPU_EARG;
    u64 f = 0, rc = 0;
    for (size_t i = 0; i < n; i++) {
        const int b = kmer_base2(kmer[i]);
        if (b < 0) return NAF_GPU_EARG;
        f = (f << 2) | (u64)b;
        rc |= (u64)(3 - b) << (2 * i);
    }
    *k = (unsigned)n; *index = canonical && rc < f ? rc : f;
    return 0;
}
extern "C" int naf_gpu_kmer_text(unsigned k, uint64_t index, char out[13])
{
    if (!out || k < 1 || k > KMER_MAX_K || index >> (2 * k)) return NAF_GPU_EARG;
    for (unsigned i = 0; i < k; i++) out[i] = "ACGT"[(index >> (2 * (k - 1 - i))) & 3];
    out[k] = 0;
    return 0;
}

// rows_only: the sizes, from the lengths alone.  Otherwise the tables go to d_counts (count_cap counters) and, with PER_RECORD and a d_rows,
// the rows to d_rows (row_cap rows); too small a capacity is found before anything is written.
static int kmers_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, unsigned K, int flags, u64 first, u64 count, u64 *d_counts, size_t count_cap,
                     u8 *d_rows, size_t row_cap, u64 *n_rows, u64 *n_counters, naf_gpu_kmer_row *h_total, bool rows_only)
{
    if (!c || !d_naf || !n_rows || !n_counters) return NAF_GPU_EARG;
    *n_rows = 0; *n_counters = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    if (K < 1 || K > KMER_MAX_K) return ctx_fail(c, NAF_GPU_EARG, "kmers: k %u: a k-mer has 1 to %u bases", K, KMER_MAX_K);
    if (flags & ~(int)KMER_FLAGS) return ctx_fail(c, NAF_GPU_EARG, "kmers: flags %d: only bits 0 (NAF_GPU_KMER_CANONICAL) and 1 (NAF_GPU_KMER_PER_RECORD) are defined", flags);
    if (!rows_only && ((uintptr_t)d_counts & 7)) return ctx_fail(c, NAF_GPU_EARG, "kmers: d_counts %p is not 8-byte aligned", (void *)d_counts);
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, "kmers", "k-mers cannot be counted", first, &count, pl);
    if (rc) return rc;
    if (!pl.h.n_sequences) return 0;                                              // no records: no tables
    const bool per = (flags & NAF_GPU_KMER_PER_RECORD) != 0, canon = (flags & NAF_GPU_KMER_CANONICAL) != 0;
    const u64 nk = 1ull << (2 * K), rows = per ? count : 1;
    if (rows > (~0ull >> (2 * K)) / 8) return ctx_fail(c, NAF_GPU_EARG, "kmers: %llu tables of 4^%u counters are too many", (unsigned long long)rows, K);
    *n_rows = rows; *n_counters = rows * nk;
    if (rows_only) return 0;
    const bool want_rows = per && d_rows;
    if (rows * nk > count_cap || (want_rows && rows > row_cap))
        return ctx_fail(c, NAF_GPU_ECAP, "kmers: %llu counters and %llu rows, capacity %zu and %zu", (unsigned long long)(rows * nk), (unsigned long long)(want_rows ? rows : 0), count_cap,
                        want_rows ? row_cap : (size_t)0);
    if (!rows) return 0;
    if (!d_counts) return ctx_fail(c, NAF_GPU_EARG, "kmers: no place for the counts (d_counts is NULL)");
    HIP_TRY(c, hipMemsetAsync(d_counts, 0, rows * nk * 8, c->stream));
    if (!count) { HIP_TRY(c, hipStreamSynchronize(c->stream)); return 0; }       // an empty selection: one table of zeros
    const EmitP &P = pl.P;

    // [0] positions, [1] counted of all rows, [2] / [3] tiles of the two paths, [4 ..] counted per row
    u64 *d_sum = arena_new<u64>(c, 4 + rows); if (!d_sum) return NAF_GPU_ENOMEM;
    HIP_TRY(c, hipMemsetAsync(d_sum, 0, (4 + rows) * 8, c->stream));
    std::vector<RecPiece> pieces;
    if ((rc = piece_plan(c, P, first, count, "KMERS_PIECE", KMER_PIECE_DEFAULT, pieces))) return rc;
    u32 lds_k = KMER_LDS_K_DEFAULT;
    { const char *e = ctx_opt(c, "KMERS_LDS_K"); if (e && e[0] >= '0' && e[0] <= '7' && !e[1]) lds_k = (u32)(e[0] - '0'); }
    const bool lds_on = K <= lds_k, tracing = ctx_tracing(c);
    const u32 entries = lds_on ? (u32)nk * (K <= 3 ? 64u : 1u) : 0u;             // words of LDS: 16 KiB at K = 3 and K = 6, 64 KiB at K = 7
    const u32 chunk = entries / 64 > 16 ? entries / 64 : 16;                      // tiles a workgroup: 16 .. 256, so that a flush is a small part of it

    PieceSweep sw(c, d_naf, pl, "kmers");
    for (const RecPiece &pc : pieces) {
        if (pc.p_hi == pc.p_lo) continue;
        PieceSweep::Tiles tl;
        if ((rc = sw.seq_for(pc, KMER_TILE, &tl))) return rc;
        LAUNCH(c, "unnaf_kmer_count", k_kmer_count, (u32)((tl.ntiles + chunk - 1) / chunk), 64, entries * 4, tl.seq, tl.b_hi, P.rec_base, first, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0,
               tl.ntiles, chunk, (u32)K, canon ? 1u : 0u, per ? 1u : 0u, lds_on ? 1u : 0u, (unsigned long long *)d_counts, (unsigned long long *)d_sum + 4,
               tracing ? (unsigned long long *)d_sum + 2 : (unsigned long long *)nullptr);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        sw.release();
    }
    { const u64 nb = (count + 255) / 256;
      LAUNCH(c, "unnaf_kmer_rows", k_kmer_rows, (u32)(nb < 2048 ? nb : 2048), 256, 0, P.rec_base, first, count, (u32)K, per ? (const u64 *)d_sum + 4 : (const u64 *)nullptr,
             want_rows ? d_rows : (u8 *)nullptr, (unsigned long long *)d_sum); }
    HIP_TRY(c, hipGetLastError());
    u64 sum[5];
    if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc;
    if (h_total) {
        h_total->record = count; h_total->begin = 0; h_total->end = pieces.back().p_hi - pieces.front().p_lo;
        h_total->positions = sum[0]; h_total->counted = per ? sum[1] : sum[4];
    }
    if (tracing) ctx_trace(c, "[kmers] k %u rows %llu pieces %zu sequence bytes decoded %llu of %llu lds tiles %llu global tiles %llu\n", K, (unsigned long long)rows, pieces.size(),
                           (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes, (unsigned long long)sum[2], (unsigned long long)sum[3]);
    return 0;
}

extern "C" int naf_gpu_unnaf_kmers_rows(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, unsigned k, int flags, uint64_t first, uint64_t count,
                                        uint64_t *n_rows, uint64_t *n_counters)
{
    int rc = kmers_run(c, (const u8 *)d_naf, naf_len, k, flags, first, count, nullptr, 0, nullptr, 0, n_rows, n_counters, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_kmers(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, unsigned k, int flags, uint64_t first, uint64_t count,
                                   uint64_t *d_counts, size_t count_cap, naf_gpu_kmer_row *d_rows, size_t row_cap,
                                   uint64_t *n_rows, uint64_t *n_counters, naf_gpu_kmer_row *h_total)
{
    int rc = kmers_run(c, (const u8 *)d_naf, naf_len, k, flags, first, count, (u64 *)d_counts, count_cap, (u8 *)d_rows, row_cap, n_rows, n_counters, h_total, false);
    if (c) arena_settle(c);
    return rc;
}
