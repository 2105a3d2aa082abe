// screen.h -- reads screened against the k-mers of a second archive, decided in the packed 4-bit stream (naf_gpu_unnaf_screen).  Part of
// emit.hip (included by it, behind dedup.h): the front of the call, the pieces and the decode of a piece's bytes are payload.h's
// (records_front, piece_plan, PieceSweep), the loads packed.h's, the bit planes, the spread and the reversal of the 2-bit groups kmers.h's
// (kmer_planes, kmer_spread, kmer_reverse_pairs), the walk of a lane's parts (k_screen_insert), the stage of the bounds rows and the totals
// reads.h's (lane_parts, k_bounds_stage, wg_sums).  The contract is include/naf_gpu.h's.
//
// A k-mer's KEY is naf_gpu_kmer_index's index in 64 bits: two bits a base, the first base the most significant, K <= 31, so a key stays
// below 2^62 and all ones is the empty slot.  A lane holds its 64 bases and the 30 behind them (the neighbour lane's first four dwords by
// __shfl_down; behind the tile's last lane sixteen bounds-checked bytes) as the validity mask eroded by K and as M (base j at bits 2 j) and
// R (the same 96 groups in reverse order): the key of start j is a 2 K-bit window of R, that of its reverse complement the same window of
// ~M.
//
// k_screen_insert: the reference, a wavefront per tile.  Every valid start's key -- the canonical one unless FORWARD_ONLY -- goes into an
//                  open-addressing table of 8-byte slots preset to all ones (load <= 1/2): an empty slot is claimed by CAS, a slot that
//                  holds the key is done, anything else means the next slot.  A claim adds one to ref_kmers and sets the key's bit of the
//                  prefilter bitmap by atomicOr.  Which slot a key ends in depends on the order; WHICH keys the table holds, and which
//                  bits are set, does not.
// k_screen_mark:   the reads.  A workgroup of four wavefronts copies the bitmap into LDS once and then walks a chunk of tiles, a wavefront
//                  per tile.  A start whose bit is clear is no hit and touches no HBM; one whose bit is set probes the table.  The hits of
//                  a lane's part of a record go to hits[record] by ONE atomicAdd (none when there are none: integer adds have no order).
// k_screen_finish: a lane per record writes the row (5 u64, in the arena; rows_copy takes them to the caller's alignment) and adds the
//                  totals (wg_sums), the records that take part among them.
#pragma once

#define SCREEN_TILE 4096u
#define SCREEN_MAX_K 31u
#define SCREEN_ROW_U64 5u
#define SCREEN_PIECE_DEFAULT (1ull << 31)      // bases swept per decode (NAF_GPU_SCREEN_PIECE)
#define SCREEN_EMPTY 0xFFFFFFFFFFFFFFFFull
#define SCREEN_FILTER_DEFAULT (1u << 18)       // bits of the prefilter: 32 KiB of LDS a workgroup, four workgroups of four waves a CU
#define SCREEN_FILTER_MAX (1u << 19)           // 64 KiB: what a launch takes without asking for more
#define SCREEN_WAVES 4u                        // wavefronts of a k_screen_mark workgroup
#define SCREEN_CHUNK 16u                       // tiles a wavefront of it walks: 64 tiles (128 KiB of packed bytes) per copy of the bitmap
#define SCREEN_FLAGS (NAF_GPU_SCREEN_KEEP_MATCHED | NAF_GPU_SCREEN_FORWARD_ONLY)
#define SCREEN_SUMS 8u                         // reads, considered, matched, kept, bases, kept_bases, hit_kmers, (free)

// ---- the bits of a lane ------------------------------------------------------------------------------------------------------------
// e: bit j = the K bases from the lane's base j on are all stored as exactly A, C, G or T; m: base j's two bits at bits 2 j (l) and 2 j + 1
// (h) of (m2 : m1 : m0), j < 96; r: the same 96 groups in reverse order
struct ScreenLane { u64 e, m0, m1, m2, r0, r1, r2; };
// bits [s, s + 62) of the 192 bits (w2 : w1 : w0) under mask; s < 192
__device__ __forceinline__ u64 screen_window(u64 w0, u64 w1, u64 w2, u32 s, u64 mask)
{
    const u32 q = s >> 6, b = s & 63u;
    const u64 lo = q == 0 ? w0 : q == 1 ? w1 : w2, hi = q == 0 ? w1 : q == 1 ? w2 : 0ull;
    return ((lo >> b) | ((hi << 1) << (63u - b))) & mask;
}
// x: the lane's 64 bases; y: the 32 behind them (30 are looked at); K = 1 .. 31
__device__ __forceinline__ void k_screen_keys(const u32 (&x)[8], const u32 (&y)[4], u32 K, ScreenLane &s)
{
    u64 v = 0, h = 0, l = 0, ve = 0, he = 0, le = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { u32 a, b, c; kmer_planes(x[i], a, b, c); v |= (u64)a << (8 * i); h |= (u64)b << (8 * i); l |= (u64)c << (8 * i); }
#pragma unroll
    for (int i = 0; i < 4; i++) { u32 a, b, c; kmer_planes(y[i], a, b, c); ve |= (u64)a << (8 * i); he |= (u64)b << (8 * i); le |= (u64)c << (8 * i); }
    for (u32 w = 1; w < K; ) {                                                    // the erosion of kmers.h over 96 bits
        const u32 t = w < K - w ? w : K - w;                                      // 1 .. 16
        v &= (v >> t) | (ve << (64 - t)); ve &= ve >> t; w += t;
    }
    s.e = v;
    s.m0 = (kmer_spread((u32)h) << 1) | kmer_spread((u32)l); s.m1 = (kmer_spread((u32)(h >> 32)) << 1) | kmer_spread((u32)(l >> 32));
    s.m2 = (kmer_spread((u32)he) << 1) | kmer_spread((u32)le);
    s.r0 = kmer_reverse_pairs(s.m2); s.r1 = kmer_reverse_pairs(s.m1); s.r2 = kmer_reverse_pairs(s.m0);
}
// the key of the k-mer at start j of the lane (bit j of e is set); mask = 4^K - 1
__device__ __forceinline__ u64 screen_key_at(const ScreenLane &s, u32 j, u32 K, u64 mask, bool canon)
{
    const u64 f = screen_window(s.r0, s.r1, s.r2, 2u * (96u - j - K), mask);
    if (!canon) return f;
    const u64 rc = screen_window(~s.m0, ~s.m1, ~s.m2, 2u * j, mask);
    return f < rc ? f : rc;
}
__device__ __forceinline__ u64 screen_mix(u64 x)
{
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}
// the key's bit of a bitmap of fbits bits (a power of two, at most 2^24): bits of the hash the slot number does not use
__device__ __forceinline__ u32 screen_filter_bit(u64 hm, u32 fbits) { return (u32)(hm >> 40) & (fbits - 1u); }
// The 32 bases behind a lane's 64.  Every lane of the wave calls it (four shuffles): x = what packed_load64 gave it, zeros in a lane that
// is not `active`; lane 63 reads the bytes from (g >> 1) + 32 on that lie in front of b_end.
__device__ __forceinline__ void screen_behind(const u8 *seq, u64 b_end, u64 g, bool active, u32 lane, const u32 (&x)[8], u32 (&y)[4])
{
    u32 w[4] = { 0, 0, 0, 0 };
    if (active && lane == 63) packed_tail<4>(seq, b_end, (g >> 1) + 32, w);
#pragma unroll
    for (int i = 0; i < 4; i++) { const u32 d = (u32)__shfl_down((int)x[i], 1); y[i] = lane != 63 ? d : w[i]; }
}
// ---- end of the bits of a lane -----------------------------------------------------------------------------------------------------

struct ScreenP : ReadsPiece {
    u64 first;                                 // win, part and hits: [0] is record first's (the reads; not looked at by k_screen_insert)
    const u64 *win; const u8 *part;
    unsigned long long *hits;
    unsigned long long *tab; u64 slots, cut;   // the table; the mask of NAF_GPU_SCREEN_HASH_BITS
    u32 *filter; u32 fbits;                    // the bitmap in HBM, its bits (0: no prefilter)
    unsigned long long *ctr;                   // insert: [0] valid starts, [1] claims; mark: [2] valid starts, [3] filtered, [4] probed
    u32 K, canon;
};

__global__ __launch_bounds__(64) void k_screen_insert(ScreenP P)
{
    const u32 lane = threadIdx.x;
    const u64 tile = xcd_block();
    const u64 g = P.t0 + tile * SCREEN_TILE + lane * 64;
    const u64 lo = g > P.p_lo ? g : P.p_lo, hi = g + 64 < P.p_hi ? g + 64 : P.p_hi;
    const bool active = g < P.p_hi && lo < hi;
    const u32 K = P.K; const u64 mask = (1ull << (2 * K)) - 1;
    u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, y[4];
    if (active) packed_load64(P.seq, P.b_end, g, x);
    screen_behind(P.seq, P.b_end, g, active, lane, x, y);
    u32 n_valid = 0, n_claims = 0;
    if (active) {
        ScreenLane S;
        k_screen_keys(x, y, K, S);
        if (S.e) {
            lane_parts(P.rec_base, P.r_lo, P.r_hi, lo, hi, [&](u64, u64, u64 rend, u64 pos, u64 stop) {     // the part: bases [pos, stop) of a record
                const u64 lim = rend + 1 > K ? rend + 1 - K : 0, ub = lim < stop ? lim : stop;     // no k-mer over the record's end
                if (pos < ub) {
                    const u64 m = S.e & kmer_bits((u32)(pos - g), (u32)(ub - g));
                    n_valid += (u32)__popcll(m);
                    for (u64 p = m; p; p &= p - 1) {
                        const u64 key = screen_key_at(S, (u32)__builtin_ctzll(p), K, mask, P.canon != 0);
                        const u64 hm = screen_mix(key);
                        u64 i = hm & P.cut & (P.slots - 1);
                        for (u64 n = 0; n < P.slots; n++, i = (i + 1) & (P.slots - 1)) {
                            unsigned long long cur = __hip_atomic_load(&P.tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (cur == SCREEN_EMPTY) {
                                cur = atomicCAS(&P.tab[i], SCREEN_EMPTY, (unsigned long long)key);
                                if (cur == SCREEN_EMPTY) {
                                    n_claims++;
                                    if (P.fbits) { const u32 b = screen_filter_bit(hm, P.fbits); atomicOr(&P.filter[b >> 5], 1u << (b & 31u)); }
                                    break;
                                }
                            }
                            if (cur == key) break;
                        }
                    }
                }
            });
        }
    }
    const u32 sv = wave_sum_u32(n_valid), sc = wave_sum_u32(n_claims);
    if (lane == 0 && sv) atomicAdd(&P.ctr[0], (unsigned long long)sv);
    if (lane == 0 && sc) atomicAdd(&P.ctr[1], (unsigned long long)sc);
}

// chunk: tiles a wavefront walks; the launch has fbits / 8 bytes of dynamic LDS
__global__ __launch_bounds__(64 * SCREEN_WAVES) void k_screen_mark(ScreenP P, u32 chunk)
{
    extern __shared__ u32 screen_bits[];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (P.fbits) {
        for (u32 w = tid; w < P.fbits / 32; w += 64 * SCREEN_WAVES) screen_bits[w] = P.filter[w];
        __syncthreads();
    }
    const u32 K = P.K; const u64 mask = (1ull << (2 * K)) - 1;
    const u64 tb = (u64)xcd_block() * chunk * SCREEN_WAVES, te = tb + (u64)chunk * SCREEN_WAVES < P.ntiles ? tb + (u64)chunk * SCREEN_WAVES : P.ntiles;
    u32 n_valid = 0, n_filtered = 0, n_probed = 0;                                // (a wavefront walks at most 2^26 bases of a launch: chunk <= 2^14)
    for (u64 t = tb + wave; t < te; t += SCREEN_WAVES) {
        const u64 g = P.t0 + t * SCREEN_TILE + lane * 64;                         // the lane's first base
        const u64 lo = g > P.p_lo ? g : P.p_lo, hi = g + 64 < P.p_hi ? g + 64 : P.p_hi;   // the bases of it that are swept
        const bool active = g < P.p_hi && lo < hi;
        u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, y[4];
        if (active) packed_load64(P.seq, P.b_end, g, x);
        screen_behind(P.seq, P.b_end, g, active, lane, x, y);
        if (!active) continue;
        ScreenLane S;
        k_screen_keys(x, y, K, S);
        if (!S.e) continue;                                                       // no valid start in the lane: no walk
        // (lane_parts' walk, written out: through the helper this kernel took 1.3 to 3 % longer)
        u64 r = upper_bound_u64(P.rec_base, P.r_lo, P.r_hi + 1, lo) - 1;          // rec_base[r] <= lo < rec_base[r + 1]
        u64 rbase = P.rec_base[r], rend = P.rec_base[r + 1], pos = lo;
        for (;;) {
            const u64 stop = rend < hi ? rend : hi;                               // the part: bases [pos, stop) of record r
            const u64 k = r - P.first;
            if (P.part[k]) {
                const u64 wb = rbase + P.win[2 * k], we = rbase + P.win[2 * k + 1];
                if (we - wb >= K) {                                               // starts [wb, we - K] of the window, those of this part
                    const u64 ua = pos > wb ? pos : wb, ub = stop < we - K + 1 ? stop : we - K + 1;
                    if (ua < ub) {
                        const u64 m = S.e & kmer_bits((u32)(ua - g), (u32)(ub - g));
                        n_valid += (u32)__popcll(m);
                        u32 hits = 0;
                        for (u64 p = m; p; p &= p - 1) {
                            const u64 key = screen_key_at(S, (u32)__builtin_ctzll(p), K, mask, P.canon != 0);
                            const u64 hm = screen_mix(key);
                            if (P.fbits) {
                                const u32 b = screen_filter_bit(hm, P.fbits);
                                if (!((screen_bits[b >> 5] >> (b & 31u)) & 1u)) { n_filtered++; continue; }
                            }
                            n_probed++;
                            u64 i = hm & P.cut & (P.slots - 1);
                            for (u64 n = 0; n < P.slots; n++, i = (i + 1) & (P.slots - 1)) {
                                const u64 cur = P.tab[i];
                                if (cur == key) { hits++; break; }
                                if (cur == SCREEN_EMPTY) break;
                            }
                        }
                        if (hits) atomicAdd(&P.hits[k], (unsigned long long)hits);
                    }
                }
            }
            pos = stop;
            if (stop >= hi) break;
            do { r++; rbase = rend; rend = P.rec_base[r + 1]; } while (rend <= pos);      // the next record that has bases (pos < hi <= p_hi: there is one)
        }
    }
    const u32 sv = wave_sum_u32(n_valid), sf = wave_sum_u32(n_filtered), sp = wave_sum_u32(n_probed);
    if (lane == 0 && sv) atomicAdd(&P.ctr[2], (unsigned long long)sv);
    if (lane == 0 && sf) atomicAdd(&P.ctr[3], (unsigned long long)sf);
    if (lane == 0 && sp) atomicAdd(&P.ctr[4], (unsigned long long)sp);
}

struct ScreenFinP {
    const u64 *win; const u32 *wflags; const u8 *part; const unsigned long long *hits;
    u64 first, count, min_hits; u32 keep_matched;
    u64 *rows;                                 // row of record `first` (5 u64 a row, 8-byte aligned), null: not wanted
    unsigned long long *sums;                  // SCREEN_SUMS counters
};

__global__ __launch_bounds__(256) void k_screen_finish(ScreenFinP P)
{
    __shared__ unsigned long long tsum[SCREEN_SUMS];
    const u32 tid = threadIdx.x;
    if (tid < SCREEN_SUMS) tsum[tid] = 0;
    __syncthreads();
    u64 T[SCREEN_SUMS]; for (u32 i = 0; i < SCREEN_SUMS; i++) T[i] = 0;
    const u64 k = (u64)blockIdx.x * 256 + tid;
    if (k < P.count) {
        const u64 begin = P.win[2 * k], end = P.win[2 * k + 1];
        u64 hits = 0; u32 flags = P.wflags[k];
        T[0] = 1;
        if (P.part[k]) {
            hits = P.hits[k];
            const bool matched = hits >= P.min_hits, kept = matched == (P.keep_matched != 0);
            flags = (matched ? NAF_GPU_SCREEN_MATCHED : 0u) | (kept ? NAF_GPU_TRIM_KEPT : 0u) | (flags & NAF_GPU_CLIP_CLIPPED);
            T[1] = 1; T[2] = matched; T[3] = kept; T[4] = end - begin; T[5] = kept ? end - begin : 0; T[6] = hits;
        }
        if (P.rows) { u64 *o = P.rows + k * SCREEN_ROW_U64; o[0] = P.first + k; o[1] = begin; o[2] = end; o[3] = hits; o[4] = (u64)flags; }
    }
    wg_sums(T, tsum, P.sums);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_unnaf_screen(naf_gpu_ctx *c, const void *d_naf_, size_t naf_len, const void *d_ref_, size_t ref_len, const naf_gpu_screen_opts *o,
                                    uint64_t first, uint64_t count, const void *d_bounds_, naf_gpu_screen_row *d_rows_, size_t row_cap, uint64_t *n_records,
                                    naf_gpu_screen_total *h_total)
{
    static const char who[] = "screen", who_ref[] = "screen reference", cannot[] = "reads cannot be screened";
    const u8 *d_naf = (const u8 *)d_naf_, *d_ref = (const u8 *)d_ref_, *d_bounds = (const u8 *)d_bounds_; u8 *d_rows = (u8 *)d_rows_;
    if (!c || !d_naf || !d_ref || !o || !n_records) return NAF_GPU_EARG;
    *n_records = 0;
    if (h_total) memset(h_total, 0, sizeof *h_total);
    const u32 K = o->k;
    if (K < 1 || K > SCREEN_MAX_K) return ctx_fail(c, NAF_GPU_EARG, "%s: k %u: a k-mer has 1 to %u bases", who, K, SCREEN_MAX_K);
    if (o->min_hits == 0) return ctx_fail(c, NAF_GPU_EARG, "%s: min_hits 0 (a matched read has at least one hit)", who);
    if (o->flags & ~(uint32_t)SCREEN_FLAGS) return ctx_fail(c, NAF_GPU_EARG, "%s: flags %u (NAF_GPU_SCREEN_KEEP_MATCHED, NAF_GPU_SCREEN_FORWARD_ONLY or 0)", who, (unsigned)o->flags);
    if (o->bounds_kind > NAF_GPU_SCREEN_BOUNDS_DEDUP)
        return ctx_fail(c, NAF_GPU_EARG, "%s: bounds_kind %u (NAF_GPU_SCREEN_BOUNDS_TRIM, NAF_GPU_SCREEN_BOUNDS_CLIP or NAF_GPU_SCREEN_BOUNDS_DEDUP)", who, (unsigned)o->bounds_kind);
    u64 bits = 64, fbits64 = SCREEN_FILTER_DEFAULT; bool fbits_set = false;
    if (!lever_u64(c, "SCREEN_HASH_BITS", 64, nullptr, &bits)) return ctx_fail(c, NAF_GPU_EARG, "%s: NAF_GPU_SCREEN_HASH_BITS %s (0 to 64)", who, ctx_opt(c, "SCREEN_HASH_BITS"));
    if (!lever_u64(c, "SCREEN_FILTER_BITS", SCREEN_FILTER_MAX, &fbits_set, &fbits64) || (fbits64 > 0 && (fbits64 < 64 || (fbits64 & (fbits64 - 1)))))
        return ctx_fail(c, NAF_GPU_EARG, "%s: NAF_GPU_SCREEN_FILTER_BITS %s (0, or a power of two from 64 to %u)", who, ctx_opt(c, "SCREEN_FILTER_BITS"), SCREEN_FILTER_MAX);
    u32 fbits = (u32)fbits64;
    const u32 stride = o->bounds_kind == NAF_GPU_SCREEN_BOUNDS_DEDUP ? 48u : 40u;
    const u32 flags_at = o->bounds_kind == NAF_GPU_SCREEN_BOUNDS_DEDUP ? 40u : o->bounds_kind == NAF_GPU_SCREEN_BOUNDS_CLIP ? 36u : 32u;
    UnnafPlan pl, rp;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, who, cannot, first, &count, pl);
    u64 ref_count = NAF_GPU_WHOLE;
    if (!rc) rc = records_front(c, d_ref, ref_len, FRONT_4BIT, who_ref, cannot, 0, &ref_count, rp, false);
    if (rc) { arena_settle(c); return rc; }
    *n_records = count;
    auto run = [&]() -> int {
        const EmitP &P = pl.P, &R = rp.P;
        if (d_rows && count > row_cap) return cap_fail(c, who, "rows", count, row_cap);
        LAUNCH_LIMIT(c, count, SCREEN_ROW_U64, "%s: %llu records are too many for one launch", who, (unsigned long long)count);
        const u32 grid = (u32)((count + 255) / 256);
        // [0]: the bad bounds row; [2 .. 4): the reference's valid starts and claims; [4 .. 7): the reads' valid starts, filtered, probed; [8 ..): the sums
        unsigned long long *ctr = arena_new<unsigned long long>(c, 8 + SCREEN_SUMS); if (!ctr) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(ctr, 0, (8 + SCREEN_SUMS) * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(ctr, 0xFF, 8, c->stream));
        u64 *win = nullptr; u32 *wflags = nullptr; u8 *part = nullptr; unsigned long long *hits = nullptr;
        if (count) {
            win = arena_new<u64>(c, 2 * count); wflags = arena_new<u32>(c, count); part = arena_new<u8>(c, count); hits = arena_new<unsigned long long>(c, count);
            if (!win || !wflags || !part || !hits) return NAF_GPU_ENOMEM;
            HIP_TRY(c, hipMemsetAsync(hits, 0, count * 8, c->stream));
            LAUNCH(c, "unnaf_screen_stage", k_bounds_stage, grid, 256, 0, d_bounds, stride, flags_at, ~0u, P.rec_base, first, count, win, wflags, part, ctr);
            u64 bad = 0;
            if ((rc = ctx_readback(c, &bad, ctr, 8))) return rc;
            if (bad != BOUNDS_OK) { *n_records = 0; return bounds_row_fail(c, who, bad); }
        }
        // the set: the table and the bitmap stay for the call, the reference's bytes go piece by piece
        std::vector<RecPiece> ref_pieces;
        u64 ref_bases = 0;
        if (ref_count) {
            if ((rc = piece_plan(c, R, 0, ref_count, "SCREEN_PIECE", SCREEN_PIECE_DEFAULT, ref_pieces))) return rc;
            ref_bases = ref_pieces.back().p_hi;
        }
        u64 slots = 64; while (slots < 2 * ref_bases) slots <<= 1;
        unsigned long long *tab = arena_new<unsigned long long>(c, slots);
        if (!tab) return ctx_fail(c, NAF_GPU_ENOMEM, "%s: no memory for the table of %llu slots (%llu bytes) that holds the reference's k-mers", who, (unsigned long long)slots, (unsigned long long)(slots * 8));
        u32 *filter = arena_new<u32>(c, fbits ? fbits / 32 : 1); if (!filter) return NAF_GPU_ENOMEM;
        HIP_TRY(c, hipMemsetAsync(tab, 0xFF, slots * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(filter, 0, fbits ? fbits / 8 : 4, c->stream));
        ScreenP Q; memset(&Q, 0, sizeof Q);
        Q.tab = tab; Q.slots = slots; Q.cut = bits >= 64 ? ~0ull : (1ull << bits) - 1; Q.filter = filter; Q.fbits = fbits; Q.K = K;
        Q.canon = (o->flags & NAF_GPU_SCREEN_FORWARD_ONLY) ? 0u : 1u;
        u64 decoded = 0;
        {
            PieceSweep sw(c, d_ref, rp, who_ref);
            Q.ctr = ctr + 2;
            for (const RecPiece &pc : ref_pieces) {
                if (pc.p_hi == pc.p_lo) continue;
                PieceSweep::Tiles tl;
                if ((rc = sw.seq_for(pc, SCREEN_TILE, &tl))) return rc;
                (ReadsPiece &)Q = ReadsPiece(R, pc, tl);
                LAUNCH(c, "unnaf_screen_insert", k_screen_insert, (u32)tl.ntiles, 64, 0, Q);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                sw.release();
            }
        }
        // A bitmap with more than half as many keys as bits lets most starts through and still costs its LDS (four waves a SIMD instead of
        // seven) and its copy: measured 1.3 times SLOWER than no bitmap when it is full.  Unless the lever asks for a size,
        // the reads' sweep then goes without.
        if (fbits && !fbits_set) {
            u64 claims = 0;
            if ((rc = ctx_readback(c, &claims, ctr + 3, 8))) return rc;
            if (2 * claims > fbits) fbits = 0;
        }
        Q.fbits = fbits;
        if (count) {
            std::vector<RecPiece> pieces;
            if ((rc = piece_plan(c, P, first, count, "SCREEN_PIECE", SCREEN_PIECE_DEFAULT, pieces))) return rc;
            PieceSweep sw(c, d_naf, pl, who);
            Q.ctr = ctr + 2; Q.first = first; Q.win = win; Q.part = part; Q.hits = hits;
            for (const RecPiece &pc : pieces) {
                if (pc.p_hi == pc.p_lo) continue;
                PieceSweep::Tiles tl;
                if ((rc = sw.seq_for(pc, SCREEN_TILE, &tl))) return rc;
                (ReadsPiece &)Q = ReadsPiece(P, pc, tl);
                const u64 per = (u64)SCREEN_CHUNK * SCREEN_WAVES;
                LAUNCH(c, "unnaf_screen_mark", k_screen_mark, (u32)((tl.ntiles + per - 1) / per), 64 * SCREEN_WAVES, fbits / 8, Q, SCREEN_CHUNK);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                sw.release();
            }
            decoded = sw.decoded;
            ScreenFinP F; memset(&F, 0, sizeof F);
            F.win = win; F.wflags = wflags; F.part = part; F.hits = hits; F.first = first; F.count = count; F.min_hits = o->min_hits;
            F.keep_matched = (o->flags & NAF_GPU_SCREEN_KEEP_MATCHED) ? 1u : 0u; F.sums = ctr + 8;
            if (d_rows && (rc = rows_out(c, &F.rows, count, SCREEN_ROW_U64))) return rc;
            LAUNCH(c, "unnaf_screen_finish", k_screen_finish, grid, 256, 0, F);
            if (d_rows) rows_copy(c, "unnaf_row_copy", F.rows, d_rows, count, SCREEN_ROW_U64);
            HIP_TRY(c, hipGetLastError());
        }
        u64 sum[8 + SCREEN_SUMS];
        if ((rc = ctx_readback(c, sum, ctr, sizeof sum))) return rc;
        if (h_total) { h_total->reads = sum[8]; h_total->considered = sum[9]; h_total->matched = sum[10]; h_total->kept = sum[11]; h_total->bases = sum[12];
                       h_total->kept_bases = sum[13]; h_total->kmers = sum[4]; h_total->hit_kmers = sum[14]; h_total->ref_records = ref_count; h_total->ref_bases = ref_bases;
                       h_total->ref_positions = sum[2]; h_total->ref_kmers = sum[3]; }
        if (ctx_tracing(c)) ctx_trace(c, "[screen] k %u ref records %llu ref kmers %llu of %llu slots %llu filter bits %u reads %llu considered %llu matched %llu filtered %llu probed %llu sequence bytes decoded %llu of %llu\n",
                                      K, (unsigned long long)ref_count, (unsigned long long)sum[3], (unsigned long long)sum[2], (unsigned long long)slots, fbits, (unsigned long long)count,
                                      (unsigned long long)sum[9], (unsigned long long)sum[10], (unsigned long long)sum[5], (unsigned long long)sum[6], (unsigned long long)decoded,
                                      (unsigned long long)pl.seq_bytes);
        return 0;
    };
    rc = run();
    if (rc && h_total) memset(h_total, 0, sizeof *h_total);
    arena_settle(c);
    return rc;
}
