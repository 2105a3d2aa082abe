// orfs.h -- open reading frames on the six frames of every record, listed from the packed 4-bit stream (naf_gpu_parse_codon_set,
// naf_gpu_unnaf_orfs_count, naf_gpu_unnaf_orfs).  Part of emit.hip (included by it, behind kmers.h): the front of the call, the pieces,
// the decode of a piece's bytes and count-then-write are payload.h's; the lane's 64 bases and the ones behind them are packed.h's; the bit
// planes are kmers.h's and runs.h's; this file holds the codon-set parser, the kernels and their launches.
//
// The contract (include/naf_gpu.h carries it too):
//   codon set  bit i = the codon of index i under naf_gpu_kmer_index at K = 3 (TAA 48, TAG 50, TGA 56, ATG 14).
//   known      three consecutive bases of ONE record, each stored as exactly A, C, G or T/U; any other code makes the codon unknown, and
//              an unknown codon is never a stop and never a start.  The mask plays no part.
//   frames     forward: o mod 3; reverse (the record's reverse complement, then frame 1..3 -- ORFfinder's and seqkit's convention, not
//              EMBOSS's): (L - (o + 3)) mod 3.  Coordinates are always the forward ones.
//   stretch    a maximal series of consecutive in-frame codons of one record without a stop (SPLIT_UNKNOWN: and without an unknown one).
//   ORF        starts == 0: the stretch; else from its 5'-most start codon to its 3' end.  end - begin >= min_len; CLOSED: STOP3 only.
//   order      ascending (record, begin, end), then strand; the same bytes on every run and for every piece size.
//
// A stretch of one record, strand and frame lies in ONE residue class mod 3 of the stream position (its phase), so there are six lists of
// stretch bounds, strand x phase, and a stretch is what lies between two neighbours of one list.  No kernel waits for another:
//   k_orfs_mark<false>  a wavefront per tile of 4096 bases, 64 bases a lane.  kmer_planes gives validity and the two index bits of the
//                       lane's 64 bases and of the two behind them; the twelve products "base j + k is A / C / G / T" (k = 0, 1, 2) are made
//                       once, and a codon set is an OR over its members of three ANDs picked by scalar branches (the set is uniform).  The
//                       reverse strand is the host-made reverse-complement set on the same planes.  Positions are cut to [p_lo, p_hi) and
//                       two in front of every record end; the phases are 0x9249.. rotated by the lane's residue.  A record's first base is
//                       an entry of all three lists of a strand (equal starts of empty records are one entry), so every stretch has both
//                       its bounds in its list.  With starts, six more lists hold the start codons.  The counts of the twelve lists are
//                       laid out list-major, 12 x ntiles, and ONE scan gives every tile's place in every list.
//   k_orfs_mark<true>   recomputes the tiles that have entries and stores them at their ranks from a wave prefix sum: an entry is
//                       4 x position + kind (0 record start, 1 unknown codon, 2 stop), which is also its order.
//   k_orfs_keep         a lane per entry of the six bound lists: the stretch behind it from the entry and its right neighbour alone, the
//                       start codon by one binary search in the start list of its strand and phase (only for stretches that have min_len:
//                       no lane walks a stretch), min_len and CLOSED as a flag for the next scan; the sums in registers over a grid-stride
//                       loop, reduced a workgroup in front of nine atomics (one atomic a wavefront on one address cost 150 ms a genome).
//   k_orfs_pack         the kept ones, recomputed, side by side: (begin, end, record, strand / frame / flags), still list by list.
//   k_orfs_rows         a lane per kept ORF: its rank is its index in its own list plus, for each of the five others, a lower_bound of
//                       its key (begin, end, strand) -- within a list the stretches are disjoint and ordered, so begin alone is searched.
//                       That is the contract's order without a sort.
#pragma once

#define ORFS_TILE 4096u
#define ORFS_PIECE_DEFAULT (1ull << 31)      // bases swept per decode (NAF_GPU_ORFS_PIECE)
#define ORFS_FLAGS (NAF_GPU_ORF_SPLIT_UNKNOWN | NAF_GPU_ORF_CLOSED)
#define ORFS_LISTS 12u                       // 3 strand + phase: the bounds; 6 + 3 strand + phase: the start codons
#define ORFS_PH 0x9249249249249249ull        // bits j, j mod 3 == 0

struct OrfSets { u64 stop[2], start[2]; };   // [strand]: the codons as the forward planes show them

// bit j: the codon at bases j, j + 1, j + 2 is in `set`.  is[k][b]: bit j = base j + k is base b.  The same set in every lane.
__device__ __forceinline__ u64 orfs_member(const u64 (&is)[3][4], u64 set)
{
    u64 m = 0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (!((set >> (16 * a)) & 0xFFFFu)) continue;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const u32 sub = (u32)(set >> (16 * a + 4 * b)) & 15u;
            if (sub) {
                u64 in = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) if ((sub >> k) & 1u) in |= is[2][k];
                m |= is[0][a] & is[1][b] & in;
            }
        }
    }
    return m;
}

// WRITE = false: cnt[l ntiles + t] = entries of list l in tile t.
// WRITE = true:  the entries of list l of tile t at ent[off[l ntiles + t] ...], in order; a tile without entries returns at once.
// seq: pointer to packed byte 0 of the stream; bytes [p_lo / 2, b_end) of it may be read.  Records [r_lo, r_hi) are swept:
// rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0, even, <= p_lo.  S, strands, split, cap: the same in every lane.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_orfs_mark(const u8 *seq, u64 b_end, const u64 *rec_base, u64 r_lo, u64 r_hi, u64 p_lo, u64 p_hi, u64 t0, u64 ntiles,
                                                  OrfSets S, u32 strands, u32 split, u64 *cnt, const u64 *off, u64 *ent, u64 cap)
{
    const u32 lane = threadIdx.x;
    const u64 t = xcd_block();
    if (WRITE) {
        const bool has = lane < ORFS_LISTS && off[lane * ntiles + t] != off[lane * ntiles + t + 1];
        if (!__ballot(has)) return;
    }
    const u64 g = t0 + t * ORFS_TILE + lane * 64;                                 // the lane's first base
    const u64 lo = g > p_lo ? g : p_lo, hi = g + 64 < p_hi ? g + 64 : p_hi;       // the bases of it that are swept
    const bool active = g < p_hi && lo < hi;
    u32 x[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (active) packed_load64(seq, b_end, g, x);
    const u64 behind = packed_behind12(seq, b_end, g, active, lane, x);

    u64 X[2] = { 0, 0 }, ST[2] = { 0, 0 }, SP[2] = { 0, 0 }, B = 0;                // bounds (stops and unknown codons), start codons, stops; record starts
    if (active) {
        u64 v = 0, h = 0, l = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) { u32 a, b, c; kmer_planes(x[i], a, b, c); v |= (u64)a << (8 * i); h |= (u64)b << (8 * i); l |= (u64)c << (8 * i); }
        u32 ve, he, le; kmer_planes((u32)behind & 0xFFu, ve, he, le);             // the two bases behind (bits 0 and 1)
        u64 is[3][4], K = ~0ull;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const u64 vk = k ? (v >> k) | ((u64)ve << (64 - k)) : v, hk = k ? (h >> k) | ((u64)he << (64 - k)) : h, lk = k ? (l >> k) | ((u64)le << (64 - k)) : l;
            is[k][0] = vk & ~hk & ~lk; is[k][1] = vk & ~hk & lk; is[k][2] = vk & hk & ~lk; is[k][3] = vk & hk & lk;
            K &= vk;
        }
        const u64 in = kmer_bits((u32)(lo - g), (u32)(hi - g));
        u64 Cm = in;                                                              // where a codon of one record may begin
        // records that start at g + d, d < 66: a bound at d, no codon at d - 2 and d - 1 (one upper_bound, then linear; empty records share a base)
        for (u64 i = lo == p_lo ? r_lo : upper_bound_u64(rec_base, r_lo, r_hi + 1, lo - 1); i <= r_hi; i++) {
            const u64 d = rec_base[i] - g;
            if (d >= 66) break;
            if (d < 64) B |= 1ull << d;
            const u32 from = d > 2 ? (u32)d - 2 : 0u, to = d < 64 ? (u32)d : 64u;
            if (from < to) Cm &= ~kmer_bits(from, to);
        }
        B &= in;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (!((strands >> s) & 1u)) continue;
            SP[s] = orfs_member(is, S.stop[s]) & Cm;
            X[s] = split ? (SP[s] | ~K) & Cm : SP[s];
            if (S.start[s]) ST[s] = orfs_member(is, S.start[s]) & Cm;
        }
    }
    const u32 res = (u32)(g % 3);
#pragma unroll
    for (int s = 0; s < 2; s++) {
#pragma unroll
        for (int ph = 0; ph < 3; ph++) {
            const u64 PH = ORFS_PH << ((ph + 3 - res) % 3);                       // the lane's positions of stream phase ph
            const u64 xb = X[s] & PH, xs = ST[s] & PH, rb = ((strands >> s) & 1u) ? B : 0ull;
            const u32 nb = (u32)__popcll(xb) + (u32)__popcll(rb), ns = (u32)__popcll(xs);
            const u64 lb = (u64)(3 * s + ph) * ntiles + t, ls = (u64)(6 + 3 * s + ph) * ntiles + t;
            if (!WRITE) {
                const u32 tot = wave_sum_u32(nb | (ns << 16));                    // a tile has at most 8192 of either
                if (lane == 0) { cnt[lb] = tot & 0xFFFFu; cnt[ls] = tot >> 16; }
            } else {
                const u32 pre = wave_prefix_u32(nb | (ns << 16), lane);
                u64 pb = off[lb] + (pre & 0xFFFFu), ps = off[ls] + (pre >> 16);
                for (u64 m = xb | rb; m; m &= m - 1) {
                    const u32 j = (u32)__builtin_ctzll(m);
                    if ((rb >> j) & 1u) { if (pb < cap) ent[pb] = (g + j) * 4; pb++; }
                    if ((xb >> j) & 1u) { if (pb < cap) ent[pb] = (g + j) * 4 + (((SP[s] >> j) & 1u) ? 2u : 1u); pb++; }
                }
                for (u64 m = xs; m; m &= m - 1, ps++) if (ps < cap) ent[ps] = (g + (u32)__builtin_ctzll(m)) * 4;
            }
        }
    }
}

struct OrfAt { u64 begin, end; u32 oflags; bool stretch, stop; };   // stretch: the entry has a stretch of at least one codon behind it; stop: it is a stop codon
// The ORF of the stretch behind entry k of list l (0 .. 5), in stream positions; false: none, or one that the call does not keep.
// off: the scan of the mark counts (off[l ntiles] = where list l begins in ent).
__device__ __forceinline__ bool orfs_at(const u64 *ent, const u64 *off, u64 ntiles, u64 k, u32 l, u64 p_hi, u32 use_starts, u64 min_len, u32 closed, OrfAt &o)
{
    const u32 s = l / 3, ph = l % 3;
    const u64 e0 = ent[k], e1 = k + 1 < off[(u64)(l + 1) * ntiles] ? ent[k + 1] : p_hi * 4;     // behind the list's last entry: the piece's end, a record's
    const u64 pos = e0 >> 2, npos = e1 >> 2;
    const u32 kind = (u32)e0 & 3u, nkind = (u32)e1 & 3u;
    o.stop = kind == 2; o.stretch = false;
    const u64 sb = kind ? pos + 3 : pos + (ph + 3 - (u32)(pos % 3)) % 3;          // a record's first codon of this phase
    const u64 back = nkind ? 0 : ((u32)(npos % 3) + 3 - ph) % 3;                  // a record's last codon of this phase ends there
    if (npos < back + sb + 3) return false;                                       // (an empty stretch, or a record too short for a codon)
    const u64 se = npos - back;
    o.stretch = true;
    o.oflags = s == 0 ? (nkind == 2 ? NAF_GPU_ORF_STOP3 : 0u) | (kind == 2 ? NAF_GPU_ORF_STOP5 : 0u)
                      : (kind == 2 ? NAF_GPU_ORF_STOP3 : 0u) | (nkind == 2 ? NAF_GPU_ORF_STOP5 : 0u);
    if (se - sb < min_len || (closed && !(o.oflags & NAF_GPU_ORF_STOP3))) return false;
    o.begin = sb; o.end = se;
    if (use_starts) {
        const u64 a = off[(u64)(6 + l) * ntiles], b = off[(u64)(7 + l) * ntiles];
        if (s == 0) {                                                             // the first start codon at or behind sb
            const u64 j = sb ? upper_bound_u64(ent, a, b, sb * 4 - 1) : a;
            if (j >= b || (ent[j] >> 2) >= se) return false;
            o.begin = ent[j] >> 2;
        } else {                                                                  // the last one in front of se
            const u64 j = upper_bound_u64(ent, a, b, se * 4 - 1);
            if (j <= a || (ent[j - 1] >> 2) < sb) return false;
            o.end = (ent[j - 1] >> 2) + 3;
        }
        if (o.end - o.begin < min_len) return false;
    }
    return true;
}
// the list that holds entry k < off[6 ntiles]
__device__ __forceinline__ u32 orfs_list_of(const u64 *off, u64 ntiles, u64 k) { u32 l = 0; while (k >= off[(u64)(l + 1) * ntiles]) l++; return l; }
// record, frame of an ORF [begin, end) of strand s; records [r_lo, r_hi) hold it
__device__ __forceinline__ u64 orfs_record(const u64 *rec_base, u64 r_lo, u64 r_hi, u32 s, u64 begin, u64 end, u32 &frame)
{
    const u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, begin) - 1;           // the last record that starts at or before begin: the one that has it
    frame = (u32)((s == 0 ? begin - rec_base[r] : rec_base[r + 1] - end) % 3);
    return r;
}

// a lane per entry k < n of the six bound lists (grid-stride, at most 2048 workgroups): flag[k] = 1 when its stretch gives an ORF that is kept
// (flag[n] = 0: the scan's total lands there).  sum[0] += the kept bases, sum[1 + 3 strand + frame] += 1 per kept ORF, sum[7] += stretches of
// at least one codon, sum[8] += stops: a lane keeps its own nine sums, a workgroup reduces them in front of the atomics
__global__ __launch_bounds__(256) void k_orfs_keep(const u64 *ent, const u64 *off, u64 ntiles, u64 n, u64 p_hi, const u64 *rec_base, u64 r_lo, u64 r_hi,
                                                   u32 use_starts, u64 min_len, u32 closed, u64 *flag, unsigned long long *sum)
{
    __shared__ u64 part[9][4];
    u64 acc[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k <= n; k += (u64)gridDim.x * 256) {
        u64 kept = 0;
        if (k < n) {
            const u32 l = orfs_list_of(off, ntiles, k);
            OrfAt o;
            if (orfs_at(ent, off, ntiles, k, l, p_hi, use_starts, min_len, closed, o)) {
                u32 frame; orfs_record(rec_base, r_lo, r_hi, l / 3, o.begin, o.end, frame);
                kept = o.end - o.begin;
                acc[0] += kept;
#pragma unroll
                for (u32 q = 0; q < 6; q++) acc[1 + q] += 3 * (l / 3) + frame == q ? 1 : 0;      // (no indexing by a run-time value: the sums stay in registers)
            }
            acc[7] += o.stretch ? 1 : 0; acc[8] += o.stop ? 1 : 0;
        }
        flag[k] = kept ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < 9; q++) {
        const u64 v = wave_sum_u64(acc[q]);
        if ((threadIdx.x & 63) == 0) part[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const u64 v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (v) atomicAdd(&sum[threadIdx.x], (unsigned long long)v);
    }
}
// a lane per entry: a kept one, recomputed, at place flag[k] of the four tables (flag: the scan of k_orfs_keep's); meta = list | frame << 8 | flags << 16
__global__ __launch_bounds__(256) void k_orfs_pack(const u64 *ent, const u64 *off, u64 ntiles, u64 n, u64 p_hi, const u64 *rec_base, u64 r_lo, u64 r_hi,
                                                   u32 use_starts, u64 min_len, u32 closed, const u64 *flag, u64 *cb, u64 *ce, u64 *cr, u64 *cm)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n || flag[k + 1] == flag[k]) return;
    const u32 l = orfs_list_of(off, ntiles, k);
    OrfAt o;
    if (!orfs_at(ent, off, ntiles, k, l, p_hi, use_starts, min_len, closed, o)) return;   // (it was kept: it is one)
    u32 frame; const u64 r = orfs_record(rec_base, r_lo, r_hi, l / 3, o.begin, o.end, frame);
    const u64 q = flag[k];
    cb[q] = o.begin; ce[q] = o.end; cr[q] = r; cm[q] = l | (frame << 8) | (o.oflags << 16);
}
// a lane per kept ORF q < nk: its row at rows[32 (out_base + rank)], rank = its place among the kept of all six lists in (begin, end,
// strand) order.  The kept of list l are [flag[off[l ntiles]], flag[off[(l + 1) ntiles]]) of the tables.  rows: any alignment.
__global__ __launch_bounds__(256) void k_orfs_rows(const u64 *cb, const u64 *ce, const u64 *cr, const u64 *cm, u64 nk, const u64 *flag, const u64 *off, u64 ntiles,
                                                   const u64 *rec_base, u64 out_base, u8 *rows)
{
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
    if (q >= nk) return;
    const u64 ob = cb[q], oe = ce[q], r = cr[q], m = cm[q];
    const u32 l = (u32)m & 0xFFu, s = l / 3;
    u64 rank = 0;
#pragma unroll 1
    for (u32 l2 = 0; l2 < 6; l2++) {
        const u64 a = flag[off[(u64)l2 * ntiles]], b = flag[off[(u64)(l2 + 1) * ntiles]];
        if (l2 == l) { rank += q - a; continue; }
        const u64 j = ob ? upper_bound_u64(cb, a, b, ob - 1) : a;                 // the first of list l2 that begins at or behind ob
        rank += j - a;
        if (j < b && cb[j] == ob && (ce[j] < oe || (ce[j] == oe && l2 / 3 < s))) rank++;
    }
    const u64 base = rec_base[r];
    u8 *o = rows + (out_base + rank) * 32;
    st64(o, r); st64(o + 8, ob - base); st64(o + 16, oe - base); st32(o + 24, s); st32(o + 28, ((u32)(m >> 8) & 0xFFu) | ((u32)(m >> 16) << 16));
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// 0, or NAF_GPU_EARG for what is no list of codons
extern "C" int naf_gpu_parse_codon_set(const char *text, uint64_t *set)
{
    if (!text || !set || !*text) return NAF_GPU_EARG;
    u64 s = 0;
    for (const char *p = text; ; ) {
        int code[3];
        for (int i = 0; i < 3; i++) {
            if (!p[i] || p[i] == ',') return NAF_GPU_EARG;
            code[i] = base_code(p[i]);
            if (code[i] <= 0) return NAF_GPU_EARG;                                 // no letter, or the gap
        }
        p += 3;
        if (*p && *p != ',') return NAF_GPU_EARG;
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) for (int d = 0; d < 4; d++)     // base x of ACGT is bit 3 - x of a code
            if ((code[0] & (8 >> a)) && (code[1] & (8 >> b)) && (code[2] & (8 >> d))) s |= 1ull << (16 * a + 4 * b + d);
        if (!*p) break;
        p++;
    }
    *set = s;
    return 0;
}
// the set whose members are the reverse complements of those of s
static u64 orfs_revcomp_set(u64 s)
{
    u64 r = 0;
    for (u32 i = 0; i < 64; i++)
        if ((s >> i) & 1) r |= 1ull << (16 * (3 - (i & 3)) + 4 * (3 - ((i >> 2) & 3)) + (3 - (i >> 4)));
    return r;
}

// write: the rows go to d_orfs (orf_cap entries); too small a capacity is found before anything is written.
static int orfs_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, u64 stops, u64 starts, u64 min_len, int strands, int flags, u64 first, u64 count,
                    u8 *d_orfs, size_t orf_cap, u64 *n_orfs, u64 *n_bases, u64 *per_frame, bool write)
{
    if (!c || !d_naf || !n_orfs) return NAF_GPU_EARG;
    *n_orfs = 0;
    if (n_bases) *n_bases = 0;
    if (per_frame) memset(per_frame, 0, 6 * sizeof *per_frame);
    if (!stops) return ctx_fail(c, NAF_GPU_EARG, "orfs: stops is empty: a reading frame is closed by a stop codon");
    if (starts & stops) return ctx_fail(c, NAF_GPU_EARG, "orfs: starts and stops share codons (0x%016llX)", (unsigned long long)(starts & stops));
    if (!min_len) return ctx_fail(c, NAF_GPU_EARG, "orfs: min_len 0: an open reading frame has at least one codon");
    if (strands < 1 || strands > 3) return ctx_fail(c, NAF_GPU_EARG, "orfs: strands %d: 1 (forward), 2 (reverse) or 3 (both)", strands);
    if (flags & ~(int)ORFS_FLAGS) return ctx_fail(c, NAF_GPU_EARG, "orfs: flags %d: only bits 0 (NAF_GPU_ORF_SPLIT_UNKNOWN) and 1 (NAF_GPU_ORF_CLOSED) are defined", flags);
    UnnafPlan pl;
    int rc = records_front(c, d_naf, naf_len, FRONT_4BIT, "orfs", "open reading frames cannot be listed", first, &count, pl);
    if (rc || !count) return rc;
    const EmitP &P = pl.P;
    const bool tracing = ctx_tracing(c);
    const u32 split = (flags & NAF_GPU_ORF_SPLIT_UNKNOWN) ? 1u : 0u, closed = (flags & NAF_GPU_ORF_CLOSED) ? 1u : 0u, use_starts = starts ? 1u : 0u;
    OrfSets S = { { stops, orfs_revcomp_set(stops) }, { starts, orfs_revcomp_set(starts) } };
    // [0] the kept bases, [1 .. 6] the kept ORFs per strand and frame, [7] stretches, [8] stop codons
    unsigned long long *d_sum = arena_new<unsigned long long>(c, 9); if (!d_sum) return NAF_GPU_ENOMEM;
    u64 total = 0, sum[9];

    std::vector<RecPiece> pieces;
    if ((rc = piece_plan(c, P, first, count, "ORFS_PIECE", ORFS_PIECE_DEFAULT, pieces))) return rc;
    PieceSweep sw(c, d_naf, pl, "orfs");
    rc = count_then_write(sw, pieces, ORFS_TILE, { "orfs", write, orf_cap, d_sum, sizeof sum }, &total,
                          [&](const RecPiece &pc, const PieceSweep::Tiles &tl, bool writing, u64 before, u64 *here) -> int {
        const u64 ntiles = tl.ntiles, nl = ORFS_LISTS * ntiles;
        u64 *cnt = arena_new<u64>(c, nl + 2);
        if (!cnt) return ctx_fail(c, NAF_GPU_ENOMEM, "orfs: no room for the counts of %llu tiles: set NAF_GPU_ORFS_PIECE to fewer bases", (unsigned long long)ntiles);
        HIP_TRY(c, hipMemsetAsync(cnt + nl, 0, 8, c->stream));
#define ORFS_MARK(W, name, en, cap) LAUNCH(c, name, k_orfs_mark<W>, (u32)ntiles, 64, 0, tl.seq, tl.b_hi, P.rec_base, pc.r_lo, pc.r_hi, pc.p_lo, pc.p_hi, tl.t0, ntiles, \
                                           S, (u32)strands, split, cnt, (const u64 *)cnt, en, cap)
        ORFS_MARK(false, "unnaf_orfs_count", (u64 *)nullptr, (u64)0);
        int r = scan_exclusive_u64(c, cnt, nl + 1, (u64 *)nullptr); if (r) return r;
        u64 n = 0, all = 0;                                                       // the entries of the six bound lists, and of all twelve
        if ((r = ctx_readback2(c, &n, cnt + 6 * ntiles, 8, &all, cnt + nl, 8))) return r;
        if (!n) return 0;
        LAUNCH_LIMIT(c, n + 1, 1, "orfs: %llu stretch bounds are too many for one launch: set NAF_GPU_ORFS_PIECE to fewer bases", (unsigned long long)n);
        // (in random sequence three stops and one start per 64 codons of each strand: an eighth of an entry per base)
        u64 *ent = arena_new<u64>(c, all), *flag = arena_new<u64>(c, n + 2);
        if (!ent || !flag) return ctx_fail(c, NAF_GPU_ENOMEM, "orfs: no room for %llu stops, starts and record bounds of a piece of %llu bases: set NAF_GPU_ORFS_PIECE to fewer bases",
                                           (unsigned long long)all, (unsigned long long)(pc.p_hi - pc.p_lo));
        ORFS_MARK(true, "unnaf_orfs_write", ent, all);
#undef ORFS_MARK
        LAUNCH(c, "unnaf_orfs_keep", k_orfs_keep, (u32)std::min<u64>((n + 256) / 256, 2048), 256, 0, (const u64 *)ent, (const u64 *)cnt, ntiles, n, pc.p_hi, P.rec_base, pc.r_lo, pc.r_hi,
               use_starts, min_len, closed, flag, d_sum);
        if ((r = scan_exclusive_u64(c, flag, n + 1, (u64 *)nullptr))) return r;
        if ((r = ctx_readback(c, here, flag + n, 8))) return r;
        if (!writing || !*here) return 0;
        if (before + *here > orf_cap) return NAF_GPU_ECAP;
        if (!d_orfs) return ctx_fail(c, NAF_GPU_EARG, "orfs: no place for the rows (d_orfs is NULL)");
        const u64 nk = *here;
        u64 *tab = arena_new<u64>(c, 4 * nk);
        if (!tab) return ctx_fail(c, NAF_GPU_ENOMEM, "orfs: no room for %llu open reading frames of a piece: set NAF_GPU_ORFS_PIECE to fewer bases", (unsigned long long)nk);
        LAUNCH(c, "unnaf_orfs_pack", k_orfs_pack, (u32)((n + 255) / 256), 256, 0, (const u64 *)ent, (const u64 *)cnt, ntiles, n, pc.p_hi, P.rec_base, pc.r_lo, pc.r_hi,
               use_starts, min_len, closed, (const u64 *)flag, tab, tab + nk, tab + 2 * nk, tab + 3 * nk);
        LAUNCH(c, "unnaf_orfs_rows", k_orfs_rows, (u32)((nk + 255) / 256), 256, 0, (const u64 *)tab, (const u64 *)(tab + nk), (const u64 *)(tab + 2 * nk), (const u64 *)(tab + 3 * nk), nk,
               (const u64 *)flag, (const u64 *)cnt, ntiles, P.rec_base, before, d_orfs);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return 0;
    });
    *n_orfs = total;
    if (rc) return rc;
    if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc;
    if (n_bases) *n_bases = sum[0];
    if (per_frame) memcpy(per_frame, sum + 1, 6 * sizeof *per_frame);
    if (tracing) ctx_trace(c, "[orfs] orfs %llu stretches %llu stops %llu pieces %zu sequence bytes decoded %llu of %llu\n", (unsigned long long)total, (unsigned long long)sum[7],
                           (unsigned long long)sum[8], pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)pl.seq_bytes);
    return 0;
}

extern "C" int naf_gpu_unnaf_orfs_count(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t stops, uint64_t starts, uint64_t min_len, int strands, int flags,
                                        uint64_t first, uint64_t count, uint64_t *n_orfs, uint64_t *n_bases, uint64_t per_frame[6])
{
    int rc = orfs_run(c, (const u8 *)d_naf, naf_len, stops, starts, min_len, strands, flags, first, count, nullptr, 0, n_orfs, n_bases, (u64 *)per_frame, false);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_orfs(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t stops, uint64_t starts, uint64_t min_len, int strands, int flags,
                                  uint64_t first, uint64_t count, naf_gpu_orf *d_orfs, size_t orf_cap, uint64_t *n_orfs, uint64_t *n_bases)
{
    int rc = orfs_run(c, (const u8 *)d_naf, naf_len, stops, starts, min_len, strands, flags, first, count, (u8 *)d_orfs, orf_cap, n_orfs, n_bases, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
