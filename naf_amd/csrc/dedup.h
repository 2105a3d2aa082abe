// dedup.h -- exact duplicates among reads, decided in the packed 4-bit stream (naf_gpu_dedup_level, naf_gpu_unnaf_dedup).  Part of emit.hip
// (included by it, behind clip.h): the front of the call and the decode of the bytes are payload.h's (records_front, PieceSweep -- ONE
// piece: a comparison needs both records resident), the loads packed.h's, the stage of the bounds rows, the walk of a lane's parts and the
// carry of a record's parts across lanes and tiles reads.h's.  The contract is include/naf_gpu.h's.
//
// A window's SUMMARY is an element of a monoid: a polynomial hash of its codes carried with the power of its length, (h, p), h = sum of
// (code_i + 1) B^(n - 1 - i), p = B^n, two polynomials of 64 bits each (arithmetic modulo 2^64, odd bases below 2^32: a step is one
// 32 x 32 -> 64 multiply-add and one 32-bit multiply).  Two neighbouring parts combine as h = h_a p_b + h_b, p = p_a p_b; no bases are
// the identity (0, 1).  With both strands a second summary goes with it: rev = sum of (bitrev4(code_i) + 1) B^i -- the forward hash of
// the window's reverse complement -- combined the other way round, rev = rev_b p_a + rev_a.  The combine is ASSOCIATIVE, so the summary
// of a window is the same wherever the lanes and the tiles cut it: the hash of a window does not depend on the tile origin, on the
// record's place in the stream or on whether its first base is the low or the high nibble of a byte.  A record's H is (h0, h1), with
// both strands the smaller of (h0, h1) and (rev0, rev1), so a read and its reverse complement share it; every word is then cut to the
// low NAF_GPU_DEDUP_HASH_BITS bits (the lever that makes different sequences share an H on purpose).
//
// k_dedup_preset: a lane per record, behind k_bounds_stage: a record that takes no part is its own first, the others are pending; the
//                 records that take part are counted (wg_sums).
// k_dedup_hash:   a wavefront per tile of 4096 bases, 64 bases a lane, loaded once into a row of LDS; the lane walks its bases part by
//                 part (lane_parts).  Whole records finish in the lane, the others go through seam_carry; a record that crosses the tile
//                 leaves slot 0 (it began in front of the tile) or slot 1 (it ends behind it).
// k_dedup_join:   a lane per record: empty records get the identity, records of several tiles their summary from seam_join.
// k_dedup_insert: a lane per pending record into an open-addressing table of record numbers (load <= 1/2, preset to all ones): an empty
//                 slot is claimed by CAS, a slot whose occupant has the same H takes atomicMin(slot, r), any other means the next slot.
//                 A slot never changes hands to another H and a minimum does not depend on the order: every H ends with the smallest
//                 pending record that has it.
// k_dedup_verify: a pending record r finds the occupant f of its H.  r == f: a first.  Else the WINDOWS' CODES are compared, by dword
//                 with a funnel shift for odd first bases, forward and then against the bit-reversed codes from the other end.  Equal:
//                 a duplicate of f with its strand.  Not equal: r stays pending -- with all of its class, none of which equals f -- and
//                 the next round, among the pending alone, finds their true first.  A lane compares windows of up to DEDUP_LANE_MAX
//                 bases; a longer one is compared by the whole wavefront, 8 bases a lane and step.
// Rounds:         insert + verify with a fresh table until nothing is pending, one read-back a round.  The smallest pending record of
//                 every H is a first, so every round resolves at least one class; one that resolves nothing is NAF_GPU_EINTERNAL.
// k_dedup_count:  atomicAdd of one onto copies[first] per record that takes part (integers: no order).
// k_dedup_finish: a lane per record writes the row (6 u64, in the arena; rows_copy takes them to the caller's alignment) and adds the
//                 totals (wg_sums, the largest class as its one maximum) and the levels (a ballot a level).
#pragma once

#define DEDUP_TILE 4096u
#define DEDUP_ROW_U64 6u
#define DEDUP_LANE_DWORDS 9u                   // a lane's row of the staging table: its 32 bytes and one dword to spread the banks
#define DEDUP_LANE_MAX 512u                    // bases one lane compares; a longer window is the wavefront's
#define DEDUP_B0 0x9E3779B1u
#define DEDUP_B1 0x85EBCA77u
#define DEDUP_NONE 0xFFFFFFFFFFFFFFFFull       // an empty slot; a record that is pending
#define DEDUP_SUMS (8u + NAF_GPU_DEDUP_LEVELS) // reads, considered, classes, duplicates, singletons, largest, bases, kept_bases; the levels

struct DedupPow { u64 v[2][65]; };             // v[q][n] = B_q^n
static constexpr DedupPow dedup_pow_make()
{
    DedupPow t = {};
    u64 p0 = 1, p1 = 1;
    for (int n = 0; n <= 64; n++) { t.v[0][n] = p0; t.v[1][n] = p1; p0 *= DEDUP_B0; p1 *= DEDUP_B1; }
    return t;
}
__constant__ DedupPow dedup_pow = dedup_pow_make();

struct DedupSum { u64 h0, h1, p0, p1, r0, r1; };
__device__ __forceinline__ DedupSum dedup_identity() { DedupSum S; S.h0 = S.h1 = S.r0 = S.r1 = 0; S.p0 = S.p1 = 1; return S; }
// L's bases, then R's
template <bool BOTH>
__device__ __forceinline__ DedupSum dedup_combine(const DedupSum &L, const DedupSum &R)
{
    DedupSum o;
    o.h0 = L.h0 * R.p0 + R.h0; o.h1 = L.h1 * R.p1 + R.h1; o.p0 = L.p0 * R.p0; o.p1 = L.p1 * R.p1;
    if (BOTH) { o.r0 = R.r0 * L.p0 + L.r0; o.r1 = R.r1 * L.p1 + L.r1; } else { o.r0 = o.r1 = 0; }
    return o;
}
template <bool BOTH>
__device__ __forceinline__ DedupSum dedup_sum_down(const DedupSum &S, int d)
{
    DedupSum o;
    o.h0 = shfl_down_u64(S.h0, d); o.h1 = shfl_down_u64(S.h1, d); o.p0 = shfl_down_u64(S.p0, d); o.p1 = shfl_down_u64(S.p1, d);
    if (BOTH) { o.r0 = shfl_down_u64(S.r0, d); o.r1 = shfl_down_u64(S.r1, d); } else { o.r0 = o.r1 = 0; }
    return o;
}

struct DedupP : ReadsPiece {
    const u64 *win;                            // win[2k], win[2k + 1]: the window of record r_lo + k
    u64 *hash;                                 // hash[2k], hash[2k + 1]: its H
    DedupSum *open;                            // two slots a tile
    u64 cut;                                   // the mask of NAF_GPU_DEDUP_HASH_BITS
    u32 both;
};

// the H of record r from the summary of its whole window
__device__ __forceinline__ void dedup_done(const DedupP &P, u64 r, const DedupSum &S)
{
    u64 a = S.h0, b = S.h1;
    if (P.both && (S.r0 < a || (S.r0 == a && S.r1 < b))) { a = S.r0; b = S.r1; }
    P.hash[2 * (r - P.r_lo)] = a & P.cut; P.hash[2 * (r - P.r_lo) + 1] = b & P.cut;
}

// first_of[k]: k for a record that takes no part, DEDUP_NONE (pending) for the others; *considered += the others
__global__ __launch_bounds__(256) void k_dedup_preset(const u8 *part, u64 count, u64 *first_of, unsigned long long *considered)
{
    __shared__ unsigned long long tsum[1];
    if (threadIdx.x == 0) tsum[0] = 0;
    __syncthreads();
    u64 T[1] = { 0 };
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < count) { T[0] = part[k] != 0; first_of[k] = T[0] ? DEDUP_NONE : k; }
    wg_sums(T, tsum, considered);
}

template <bool BOTH>
__global__ __launch_bounds__(64) void k_dedup_hash(DedupP P)
{
    __shared__ u32 stage[64 * DEDUP_LANE_DWORDS];
    const u32 lane = threadIdx.x;
    const u64 tile = xcd_block();
    const u64 T0 = P.t0 + tile * DEDUP_TILE, g = T0 + lane * 64;                  // the tile's and the lane's first base
    const u64 lo = g > P.p_lo ? g : P.p_lo, hi = g + 64 < P.p_hi ? g + 64 : P.p_hi;   // the bases of it that are swept
    const bool active = lo < hi;
    u32 *st = stage + lane * DEDUP_LANE_DWORDS;
    DedupSum A = dedup_identity(), X = dedup_identity();
    bool has_a = false, pend = false, thru = false;                              // A: a part that ends a record of the lane in front; X: one whose record goes on; thru: X came from there too
    u64 xr = 0, xbase = 0, xend = 0;                                              // X's record
    if (active) {
        u32 x[8];
        packed_load64(P.seq, P.b_end, g, x);
#pragma unroll
        for (u32 i = 0; i < 8; i++) st[i] = x[i];                                 // (read by the lane that wrote them: no barrier)
        lane_parts(P.rec_base, P.r_lo, P.r_hi, lo, hi, [&](u64 r, u64 rbase, u64 rend, u64 at, u64 stop) {      // the part: bases [at, stop) of the stream
            const u64 wb = rbase + P.win[2 * (r - P.r_lo)], we = rbase + P.win[2 * (r - P.r_lo) + 1];
            const u64 ua = at > wb ? at : wb, ub = stop < we ? stop : we;         // its bases inside the record's window
            DedupSum S = dedup_identity();
            if (ua < ub) {
                const u32 a = (u32)(ua - g), b = (u32)(ub - g);                   // as the lane's bases [a, b), 0 <= a < b <= 64
                u64 h0 = 0, h1 = 0, r0 = 0, r1 = 0, w0 = 1, w1 = 1;
                for (u32 w = a >> 3; w <= (b - 1) >> 3; w++) {
                    const u32 j0 = a > 8 * w ? a - 8 * w : 0u, j1 = b < 8 * w + 8 ? b - 8 * w : 8u;
                    u32 word = st[w] >> (4 * j0);
#pragma unroll 1
                    for (u32 j = j0; j < j1; j++, word >>= 4) {
                        const u32 c = word & 15u;
                        h0 = h0 * DEDUP_B0 + (c + 1); h1 = h1 * DEDUP_B1 + (c + 1);
                        if (BOTH) {
                            const u32 cr = (__brev(c) >> 28) + 1;
                            r0 += cr * w0; r1 += cr * w1; w0 *= DEDUP_B0; w1 *= DEDUP_B1;
                        }
                    }
                }
                S.h0 = h0; S.h1 = h1; S.r0 = r0; S.r1 = r1; S.p0 = dedup_pow.v[0][b - a]; S.p1 = dedup_pow.v[1][b - a];
            }
            const bool from_front = rbase < at, goes_on = rend > stop;
            if (!from_front && !goes_on) dedup_done(P, r, S);
            else if (!goes_on) { A = S; has_a = true; }
            else { X = S; pend = true; thru = from_front; xr = r; xbase = rbase; xend = rend; }
        });
    }
    const bool head = seam_carry(lane, has_a, A, pend, thru, X, [](const DedupSum &S, int d) { return dedup_sum_down<BOTH>(S, d); },
                                 [](const DedupSum &L, const DedupSum &R) { return dedup_combine<BOTH>(L, R); });
    if (lane == 0 && has_a) P.open[2 * tile] = A;                                 // it came from the tile in front: the record's bases in this tile are that part
    if (head) {
        if (xbase >= T0 && xend <= T0 + DEDUP_TILE) dedup_done(P, xr, X);
        else P.open[2 * tile + (xbase < T0 ? 0 : 1)] = X;
    }
}

__global__ __launch_bounds__(256) void k_dedup_join(DedupP P)
{
    const u64 r = P.r_lo + (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= P.r_hi) return;
    const u64 rbase = P.rec_base[r], rend = P.rec_base[r + 1];
    if (rend == rbase) { dedup_done(P, r, dedup_identity()); return; }
    DedupSum S;
    const u64 tiles = P.both ? seam_join(P.open, P.t0, DEDUP_TILE, rbase, rend, S, [](const DedupSum &L, const DedupSum &R) { return dedup_combine<true>(L, R); })
                             : seam_join(P.open, P.t0, DEDUP_TILE, rbase, rend, S, [](const DedupSum &L, const DedupSum &R) { return dedup_combine<false>(L, R); });
    if (tiles > 1) dedup_done(P, r, S);
}

__device__ __forceinline__ u64 dedup_mix(u64 a, u64 b)
{
    u64 x = a ^ (b * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

// first_of[k] == DEDUP_NONE: record k of the selection is pending.  tab: `slots` (a power of two) record numbers of the selection.
__global__ __launch_bounds__(256) void k_dedup_insert(const u64 *hash, const u64 *first_of, u64 count, unsigned long long *tab, u64 slots)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= count || first_of[k] != DEDUP_NONE) return;
    const u64 a = hash[2 * k], b = hash[2 * k + 1];
    u64 i = dedup_mix(a, b) & (slots - 1);
    for (u64 n = 0; n < slots; n++, i = (i + 1) & (slots - 1)) {
        unsigned long long cur = __hip_atomic_load(&tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == DEDUP_NONE) { cur = atomicCAS(&tab[i], DEDUP_NONE, (unsigned long long)k); if (cur == DEDUP_NONE) return; }
        if (cur < count && hash[2 * cur] == a && hash[2 * cur + 1] == b) { atomicMin(&tab[i], (unsigned long long)k); return; }
    }
}

// the eight codes from base `pos` of the stream on (those at or behind byte b_end read as 0)
__device__ __forceinline__ u32 dedup_get8(const u8 *seq, u64 b_end, u64 pos)
{
    const u64 b0 = pos >> 1;
    u64 v;
    if (b0 + 8 <= b_end) v = ld64(seq + b0); else packed_tail<1>(seq, b_end, b0, &v);
    return (u32)(v >> (4 * (pos & 1)));
}
// Chunks j0, j0 + step, .. (8 bases each) of the comparison of the n bases at pa with the n bases at pb -- rc: with their reverse
// complement --: true when all of them agree.
__device__ __forceinline__ bool dedup_same(const u8 *seq, u64 b_end, u64 pa, u64 pb, u64 n, bool rc, u64 j0, u64 step)
{
    const u64 chunks = (n + 7) / 8;
    for (u64 j = j0; j < chunks; j += step) {
        const u64 rem = n - 8 * j;                                               // bases of this chunk and behind it
        u32 a = dedup_get8(seq, b_end, pa + 8 * j), b;
        if (!rc) b = dedup_get8(seq, b_end, pb + 8 * j);
        else if (rem >= 8) b = __brev(dedup_get8(seq, b_end, pb + rem - 8));      // bases pb + rem - 8 .. pb + rem - 1, the last first, every code's bits reversed
        else b = __brev(dedup_get8(seq, b_end, pb)) >> (4 * (8 - (u32)rem));      // the window's first rem bases, the last of them first
        if (rem < 8) { const u32 m = (1u << (4 * (u32)rem)) - 1; a &= m; b &= m; }
        if (a != b) return false;
    }
    return true;
}

struct DedupV {
    const u8 *seq; u64 b_end;
    const u64 *rec_base, *win, *hash; u64 r_lo, count;
    const unsigned long long *tab; u64 slots;
    u64 *first_of; u8 *strand;
    unsigned long long *ctr;                   // [2]: records resolved in this round; [3]: windows compared; [4]: an H that has no slot (never)
    u32 both;
};

__global__ __launch_bounds__(256) void k_dedup_verify(DedupV V)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    bool cmp = false;                                                             // this lane has two windows to compare
    u64 f = DEDUP_NONE, pa = 0, pb = 0, n = 0;
    bool resolved = false;
    if (k < V.count && V.first_of[k] == DEDUP_NONE) {
        const u64 a = V.hash[2 * k], b = V.hash[2 * k + 1];
        u64 i = dedup_mix(a, b) & (V.slots - 1);
        for (u64 s = 0; s < V.slots; s++, i = (i + 1) & (V.slots - 1)) {
            const u64 cur = V.tab[i];
            if (cur >= V.count) break;                                            // an empty slot: the H was never inserted
            if (V.hash[2 * cur] == a && V.hash[2 * cur + 1] == b) { f = cur; break; }
        }
        if (f == DEDUP_NONE) atomicAdd(&V.ctr[4], 1ull);
        else if (f == k) { V.first_of[k] = k; V.strand[k] = 0; resolved = true; }
        else {
            n = V.win[2 * k + 1] - V.win[2 * k];
            if (V.win[2 * f + 1] - V.win[2 * f] == n) {
                cmp = true;
                pa = V.rec_base[V.r_lo + k] + V.win[2 * k]; pb = V.rec_base[V.r_lo + f] + V.win[2 * f];
            }
        }
    }
    int same = -1;                                                                // the strand the windows agree on
    if (cmp && n <= DEDUP_LANE_MAX) {
        if (dedup_same(V.seq, V.b_end, pa, pb, n, false, 0, 1)) same = 0;
        else if (V.both && dedup_same(V.seq, V.b_end, pa, pb, n, true, 0, 1)) same = 1;
    }
    // the longer ones, one after the other, by all lanes of the wavefront
    u64 longs = __ballot(cmp && n > DEDUP_LANE_MAX);
    while (longs) {
        const int src = __builtin_ctzll(longs);
        longs &= longs - 1;
        const u64 qa = shfl_u64(pa, src), qb = shfl_u64(pb, src), qn = shfl_u64(n, src);
        int s = __ballot(!dedup_same(V.seq, V.b_end, qa, qb, qn, false, lane, 64)) == 0 ? 0 : -1;
        if (s < 0 && V.both && __ballot(!dedup_same(V.seq, V.b_end, qa, qb, qn, true, lane, 64)) == 0) s = 1;
        if ((int)lane == src) same = s;
    }
    if (same >= 0) { V.first_of[k] = f; V.strand[k] = (u8)same; resolved = true; }
    const u64 mr = __ballot(resolved), mc = __ballot(cmp);
    if (lane == 0 && mr) atomicAdd(&V.ctr[2], (unsigned long long)__popcll(mr));
    if (lane == 0 && mc) atomicAdd(&V.ctr[3], (unsigned long long)__popcll(mc));
}

__global__ __launch_bounds__(256) void k_dedup_count(const u8 *part, const u64 *first_of, u64 count, unsigned long long *copies)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < count && part[k]) atomicAdd(&copies[first_of[k]], 1ull);
}

__host__ __device__ __forceinline__ u32 dedup_level_of(u64 n)      // n >= 1
{
    return n < 10 ? (u32)n - 1 : n < 50 ? 9u : n < 100 ? 10u : n < 500 ? 11u : n < 1000 ? 12u : n < 5000 ? 13u : n < 10000 ? 14u : 15u;
}

struct DedupFinP {
    const u64 *win; const u32 *wflags; const u8 *part, *strand; const u64 *first_of; const unsigned long long *copies;
    u64 r_lo, count;
    u64 *rows;                                 // row of record r_lo (6 u64 a row, 8-byte aligned), null: not wanted
    unsigned long long *sums;                  // DEDUP_SUMS counters
};

__global__ __launch_bounds__(256) void k_dedup_finish(DedupFinP P)
{
    __shared__ unsigned long long tsum[DEDUP_SUMS];
    const u32 tid = threadIdx.x, lane = tid & 63u;
    if (tid < DEDUP_SUMS) tsum[tid] = 0;
    __syncthreads();
    u64 T[8]; for (u32 i = 0; i < 8; i++) T[i] = 0;
    u32 level = NAF_GPU_DEDUP_LEVELS;                                             // of the class this record is the first of
    const u64 k = (u64)blockIdx.x * 256 + tid;
    if (k < P.count) {
        const u64 begin = P.win[2 * k], end = P.win[2 * k + 1], f = P.first_of[k];
        u64 copies = 0; u32 flags = P.wflags[k], strand = 0;
        T[0] = 1;
        if (P.part[k]) {
            copies = P.copies[f]; strand = P.strand[k];
            flags = (f == k ? NAF_GPU_TRIM_KEPT : NAF_GPU_DEDUP_DUPLICATE) | (flags & NAF_GPU_CLIP_CLIPPED);
            T[1] = 1; T[6] = end - begin;
            if (f == k) { T[2] = 1; T[4] = copies == 1; T[5] = copies; T[7] = end - begin; level = dedup_level_of(copies); } else T[3] = 1;
        }
        if (P.rows) { u64 *o = P.rows + k * DEDUP_ROW_U64; o[0] = P.r_lo + k; o[1] = begin; o[2] = end; o[3] = P.r_lo + f; o[4] = copies; o[5] = (u64)flags | (u64)strand << 32; }
    }
    for (u32 l = 0; l < NAF_GPU_DEDUP_LEVELS; l++) {
        const u64 m = __ballot(level == l);
        if (lane == 0 && m) atomicAdd(&tsum[8 + l], (unsigned long long)__popcll(m));
    }
    wg_sums<8, 1u << 5>(T, tsum, P.sums);                                         // [5], the largest class, is a maximum (its barrier stands behind the levels' atomics too)
    if (tid >= 8 && tid < DEDUP_SUMS && tsum[tid]) atomicAdd(&P.sums[tid], tsum[tid]);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_dedup_level(uint64_t copies, unsigned *level)
{
    if (!level || copies == 0) return NAF_GPU_EARG;
    *level = dedup_level_of(copies);
    return 0;
}

extern "C" int naf_gpu_unnaf_dedup(naf_gpu_ctx *c, const void *d_naf_, size_t naf_len, const naf_gpu_dedup_opts *o, uint64_t first, uint64_t count,
                                   const void *d_bounds_, naf_gpu_dedup_row *d_rows_, size_t row_cap, uint64_t *n_records, naf_gpu_dedup_total *h_total,
                                   uint64_t *h_levels)
{
    static const char who[] = "dedup";
    const u8 *d_naf = (const u8 *)d_naf_, *d_bounds = (const u8 *)d_bounds_; u8 *d_rows = (u8 *)d_rows_;
    if (!c || !d_naf || !o || !n_records) return NAF_GPU_EARG;
    *n_records = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    if (h_levels) memset(h_levels, 0, NAF_GPU_DEDUP_LEVELS * sizeof *h_levels);
    if (o->flags & ~(uint32_t)NAF_GPU_DEDUP_BOTH_STRANDS) return ctx_fail(c, NAF_GPU_EARG, "%s: flags %u (NAF_GPU_DEDUP_BOTH_STRANDS or 0)", who, (unsigned)o->flags);
    if (o->bounds_kind != NAF_GPU_DEDUP_BOUNDS_TRIM && o->bounds_kind != NAF_GPU_DEDUP_BOUNDS_CLIP)
        return ctx_fail(c, NAF_GPU_EARG, "%s: bounds_kind %u (NAF_GPU_DEDUP_BOUNDS_TRIM or NAF_GPU_DEDUP_BOUNDS_CLIP)", who, (unsigned)o->bounds_kind);
    u64 bits = 64;
    if (!lever_u64(c, "DEDUP_HASH_BITS", 64, nullptr, &bits)) return ctx_fail(c, NAF_GPU_EARG, "%s: NAF_GPU_DEDUP_HASH_BITS %s (0 to 64)", who, ctx_opt(c, "DEDUP_HASH_BITS"));
    const bool both = (o->flags & NAF_GPU_DEDUP_BOTH_STRANDS) != 0;
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, who, "duplicates cannot be collapsed", first, &count, pl);
    if (rc) { arena_settle(c); return rc; }
    *n_records = count;
    if (!count) { arena_settle(c); return 0; }
    auto run = [&]() -> int {
        const EmitP &P = pl.P;
        if (d_rows && count > row_cap) return cap_fail(c, who, "rows", count, row_cap);
        LAUNCH_LIMIT(c, count, DEDUP_ROW_U64, "%s: %llu records are too many for one launch", who, (unsigned long long)count);
        const u32 grid = (u32)((count + 255) / 256);
        // [0]: the bad bounds row; [1]: considered; [2 .. 5): a round's counters; [8 ..): the sums
        unsigned long long *ctr = arena_new<unsigned long long>(c, 8 + DEDUP_SUMS); if (!ctr) return NAF_GPU_ENOMEM;
        u64 *win = arena_new<u64>(c, 2 * count), *hash = arena_new<u64>(c, 2 * count), *first_of = arena_new<u64>(c, count);
        unsigned long long *copies = arena_new<unsigned long long>(c, count);
        u32 *wflags = arena_new<u32>(c, count); u8 *part = arena_new<u8>(c, count), *strand = arena_new<u8>(c, count);
        if (!win || !hash || !first_of || !copies || !wflags || !part || !strand) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(ctr, 0, (8 + DEDUP_SUMS) * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(ctr, 0xFF, 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(copies, 0, count * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(strand, 0, count, c->stream));
        LAUNCH(c, "unnaf_dedup_stage", k_bounds_stage, grid, 256, 0, d_bounds, 40u, o->bounds_kind == NAF_GPU_DEDUP_BOUNDS_CLIP ? 36u : 32u, ~0u, P.rec_base, first, count, win, wflags, part, ctr);
        LAUNCH(c, "unnaf_dedup_preset", k_dedup_preset, grid, 256, 0, (const u8 *)part, count, first_of, ctr + 1);
        u64 head[2], ends[2];
        const void *src[3] = { ctr, P.rec_base + first, P.rec_base + first + count }; void *dst[3] = { head, &ends[0], &ends[1] }; const size_t nb[3] = { 16, 8, 8 };
        if ((rc = ctx_readbackv(c, 3, dst, src, nb))) return rc;
        if (head[0] != BOUNDS_OK) { *n_records = 0; return bounds_row_fail(c, who, head[0]); }
        const u64 considered = head[1];
        // the bases of all selected records as ONE piece, held for the call
        const RecPiece pc = { first, first + count, ends[0], ends[1] };
        PieceSweep sw(c, d_naf, pl, who);
        PieceSweep::Tiles tl = { nullptr, 0, 0, 0 };
        if (pc.p_hi > pc.p_lo && (rc = sw.seq_for(pc, DEDUP_TILE, &tl))) return rc;
        DedupP Q; memset(&Q, 0, sizeof Q);
        (ReadsPiece &)Q = ReadsPiece(P, pc, tl);
        Q.win = win; Q.hash = hash; Q.cut = bits >= 64 ? ~0ull : (1ull << bits) - 1; Q.both = both;
        if (Q.ntiles) {
            Q.open = arena_new<DedupSum>(c, 2 * Q.ntiles); if (!Q.open) return NAF_GPU_ENOMEM;
            if (both) LAUNCH(c, "unnaf_dedup_hash", (k_dedup_hash<true>), (u32)Q.ntiles, 64, 0, Q);
            else LAUNCH(c, "unnaf_dedup_hash", (k_dedup_hash<false>), (u32)Q.ntiles, 64, 0, Q);
        }
        LAUNCH(c, "unnaf_dedup_join", k_dedup_join, grid, 256, 0, Q);
        u64 slots_max = 64; while (slots_max < 2 * considered) slots_max <<= 1;
        unsigned long long *tab = arena_new<unsigned long long>(c, slots_max); if (!tab) return NAF_GPU_ENOMEM;
        DedupV V; memset(&V, 0, sizeof V);
        V.seq = Q.seq; V.b_end = Q.b_end; V.rec_base = P.rec_base; V.win = win; V.hash = hash; V.r_lo = first; V.count = count; V.tab = tab;
        V.first_of = first_of; V.strand = strand; V.ctr = ctr; V.both = both;
        u64 pending = considered, rounds = 0, verified = 0;
        while (pending) {
            u64 slots = 64; while (slots < 2 * pending) slots <<= 1;
            V.slots = slots;
            HIP_TRY(c, hipMemsetAsync(tab, 0xFF, slots * 8, c->stream));
            HIP_TRY(c, hipMemsetAsync(ctr + 2, 0, 3 * 8, c->stream));
            LAUNCH(c, "unnaf_dedup_insert", k_dedup_insert, grid, 256, 0, (const u64 *)hash, (const u64 *)first_of, count, tab, slots);
            LAUNCH(c, "unnaf_dedup_verify", k_dedup_verify, grid, 256, 0, V);
            u64 got[3];
            if ((rc = ctx_readback(c, got, ctr + 2, sizeof got))) return rc;
            rounds++; verified += got[1];
            if (got[2] || got[0] == 0 || got[0] > pending)
                return ctx_fail(c, NAF_GPU_EINTERNAL, "%s: round %llu resolved %llu of %llu pending records", who, (unsigned long long)rounds, (unsigned long long)got[0], (unsigned long long)pending);
            pending -= got[0];
        }
        LAUNCH(c, "unnaf_dedup_count", k_dedup_count, grid, 256, 0, (const u8 *)part, (const u64 *)first_of, count, copies);
        DedupFinP F; memset(&F, 0, sizeof F);
        F.win = win; F.wflags = wflags; F.part = part; F.strand = strand; F.first_of = first_of; F.copies = copies; F.r_lo = first; F.count = count; F.sums = ctr + 8;
        if (d_rows && (rc = rows_out(c, &F.rows, count, DEDUP_ROW_U64))) return rc;
        LAUNCH(c, "unnaf_dedup_finish", k_dedup_finish, grid, 256, 0, F);
        if (d_rows) rows_copy(c, "unnaf_row_copy", F.rows, d_rows, count, DEDUP_ROW_U64);
        HIP_TRY(c, hipGetLastError());
        u64 sum[DEDUP_SUMS];
        if ((rc = ctx_readback(c, sum, ctr + 8, sizeof sum))) return rc;
        if (h_total) { h_total->reads = sum[0]; h_total->considered = sum[1]; h_total->classes = sum[2]; h_total->duplicates = sum[3]; h_total->singletons = sum[4];
                       h_total->largest = sum[5]; h_total->bases = sum[6]; h_total->kept_bases = sum[7]; }
        if (h_levels) for (u32 l = 0; l < NAF_GPU_DEDUP_LEVELS; l++) h_levels[l] = sum[8 + l];
        if (ctx_tracing(c)) ctx_trace(c, "[dedup] records %llu considered %llu classes %llu rounds %llu verified %llu sequence bytes decoded %llu of %llu\n", (unsigned long long)count,
                                      (unsigned long long)considered, (unsigned long long)sum[2], (unsigned long long)rounds, (unsigned long long)verified,
                                      (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes);
        return 0;
    };
    rc = run();
    if (rc && h_total) memset(h_total, 0, sizeof *h_total);
    arena_settle(c);
    return rc;
}
