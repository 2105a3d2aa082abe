// quality.h -- quality statistics per read and per cycle, counted in the quality stream (naf_gpu_quality_error_table,
// naf_gpu_unnaf_quality_rows, naf_gpu_unnaf_quality).  Part of emit.hip (included by it, behind composition.h): the front of the call,
// the pieces and the decode of a piece's bytes are payload.h's (records_front -- lengths only, any sequence type --, piece_plan, PieceSweep),
// the row copy is packed.h's; this file holds the row tables, the counting kernel and its launches.  The contract is include/naf_gpu.h's.
//
// In a .naf the quality byte g belongs to base g, so rec_base / rec_len of the sequence are the record tables of the quality stream.  A row
// is 7 u64: key, n, sum, ee, n_q20, n_q30 and the u32 pair (min, max).  Record rows are initialised with key, n = rec_len and min = 255
// (k_qual_rows), cycle rows and the total row with n = 0; everything else is added by k_qual_count in one sweep over the bytes.
//
// k_qual_count: a workgroup of four wavefronts, a wavefront per tile of 4096 quality bytes, 64 bytes a lane as four 16-byte loads; tiles
// start where the ADDRESS is a multiple of 16 (t0), whatever the alignment of the stream pointer.  Lanes whose 64 bytes do not lie inside
// the decoded range (the head and the tail of a piece) load byte by byte.  The grid is bounded (QUAL_WG_PER_CU workgroups per CU) and
// persistent: workgroup b takes tiles 4 b + wave, + 4 gridDim.x, ...  A lane finds its first record with one upper_bound in rec_base and
// walks on from there, part by part (a part: the lane's bytes of one record):
//   sum, >= Q20, >= Q30, min, max   four bytes a dword: v_sad_u8, a carry-free SWAR compare (exact for all 256 byte values) and packed
//                                   16-bit min / max of the even and the odd bytes; partial parts under byte masks
//   ee                              a 256-entry u64 table in LDS, one read per byte
//   record rows                     a lane that is one part keeps its sums; lanes of one record are adjacent, so a segmented reduction
//                                   (shuffles) sums them and the segment's first lane issues the atomics.  Other parts add their own.
//   cycle rows                      bins k < K = QUAL_LDS_BINS live in a table private to the workgroup (LDS atomics) that is flushed to
//                                   the global rows -- non-zero bins only -- at the workgroup's end; bins k >= K (long reads: few reads
//                                   share a bin) go to the global rows.  A part that lies in one bin adds its sums once (whole lanes are
//                                   combined across the wave first, as for records); W < 16 walks the bytes and adds per bin; W >= 16
//                                   sums bin by bin under byte masks.
//   histogram                       per wavefront in LDS, flushed with the bins
//   total                           the lanes' running sums, reduced across the wave at the kernel's end
// LDS counters cannot wrap: a workgroup flushes after QUAL_FLUSH_ITERS rounds of 4 tiles = 2^24 bytes at the most (NAF_GPU_QUALITY_FLUSH: after
// fewer; NAF_GPU_QUALITY_GRID: fewer workgroups -- the tests' levers for the persistent loop and the flush between its rounds), so between two flushes
// a bin's n and a histogram count are <= 2^24, its byte sum <= 255 * 2^24 < 2^32 (n and sum share one u64, as do the two threshold
// counts), its ee <= 2^24 * 2^32 = 2^56.  All adds are integer adds, min and max are order-free: the rows do not depend on the order.
#pragma once

#define QUAL_TILE 4096u
#define QUAL_ROW_U64 7u
#define QUAL_WG_PER_CU 2u                       // what its registers allow (216 VGPRs: two waves a SIMD)
#define QUAL_LDS_BINS 1024u
#define QUAL_FLUSH_ITERS 1024u                // x 4 tiles x 4096 bytes = 2^24 bytes per workgroup between two flushes
#define QUAL_PIECE_DEFAULT (1ull << 31)       // quality bytes counted per decode (NAF_GPU_QUALITY_PIECE)
#define QUAL_SMALL_W 16u                      // bins narrower than this are walked byte by byte

// round_half_up(2^32 * 10^(-(b - 33) / 10)), b = 33 .. 132 (0 from 133 on); 2^32 below 33.  Computed once with 80-digit decimals.
#define QUAL_ERR_33_132 \
    4294967296ull, 3411613790ull, 2709941160ull, 2152582778ull, 1709857278ull, 1358187913ull, 1078847007ull, 856958639ull, 680706443ull, 540704347ull, \
    429496730ull, 341161379ull, 270994116ull, 215258278ull, 170985728ull, 135818791ull, 107884701ull, 85695864ull, 68070644ull, 54070435ull, \
    42949673ull, 34116138ull, 27099412ull, 21525828ull, 17098573ull, 13581879ull, 10788470ull, 8569586ull, 6807064ull, 5407043ull, \
    4294967ull, 3411614ull, 2709941ull, 2152583ull, 1709857ull, 1358188ull, 1078847ull, 856959ull, 680706ull, 540704ull, \
    429497ull, 341161ull, 270994ull, 215258ull, 170986ull, 135819ull, 107885ull, 85696ull, 68071ull, 54070ull, \
    42950ull, 34116ull, 27099ull, 21526ull, 17099ull, 13582ull, 10788ull, 8570ull, 6807ull, 5407ull, \
    4295ull, 3412ull, 2710ull, 2153ull, 1710ull, 1358ull, 1079ull, 857ull, 681ull, 541ull, \
    429ull, 341ull, 271ull, 215ull, 171ull, 136ull, 108ull, 86ull, 68ull, 54ull, \
    43ull, 34ull, 27ull, 22ull, 17ull, 14ull, 11ull, 9ull, 7ull, 5ull, \
    4ull, 3ull, 3ull, 2ull, 2ull, 1ull, 1ull, 1ull, 1ull, 1ull
static const u64 qual_err_33[100] = { QUAL_ERR_33_132 };
__device__ const u64 qual_err_33_dev[100] = { QUAL_ERR_33_132 };
NAF_HD u64 qual_err_of(const u64 *t33, u32 b) { return b < 33 ? 1ull << 32 : b < 133 ? t33[b - 33] : 0; }

struct QBin { unsigned long long ns, qq, ee; u32 mn, mx; };        // LDS: n << 32 | sum, n_q30 << 32 | n_q20, ee, min, max (32 bytes)
struct QStat { u32 n, sum, q20, q30, mn, mx; u64 ee; };
__device__ __forceinline__ void qual_zero(QStat &S) { S.n = S.sum = S.q20 = S.q30 = 0; S.mn = 255; S.mx = 0; S.ee = 0; }

typedef unsigned short qual_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 qual_pk_min(u32 a, u32 b)
{
    const qual_u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(qual_u16x2, a), __builtin_bit_cast(qual_u16x2, b));
    return __builtin_bit_cast(u32, r);
}
__device__ __forceinline__ u32 qual_pk_max(u32 a, u32 b)
{
    const qual_u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(qual_u16x2, a), __builtin_bit_cast(qual_u16x2, b));
    return __builtin_bit_cast(u32, r);
}
// all bits of the bytes of a dword whose number is < k
__device__ __forceinline__ u32 qual_bytes_below(int k) { return k <= 0 ? 0u : k >= 4 ? ~0u : ((1u << (8 * k)) - 1u); }
// bit 7 of every byte that is >= c, 1 <= c <= 128: the low seven bits plus 128 - c carry into bit 7 and never out of the byte; a byte with
// bit 7 set is >= 128 >= c
__device__ __forceinline__ u32 qual_ge(u32 x, u32 c) { return (((x & 0x7F7F7F7Fu) + (0x80u - c) * 0x01010101u) | x) & 0x80808080u; }

// S += the lane's bytes [a, b), 0 <= a < b <= 64.  FULL: a = 0, b = 64.
template <bool FULL>
__device__ __forceinline__ void qual_span(const u32 (&x)[16], int a, int b, const u64 *etab, QStat &S)
{
    u32 sum = 0, c20 = 0, c30 = 0, mn0 = 0x00FF00FFu, mn1 = 0x00FF00FFu, mx0 = 0, mx1 = 0;
    u64 ee = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const u32 m = FULL ? ~0u : qual_bytes_below(b - 4 * i) & ~qual_bytes_below(a - 4 * i);
        const u32 y = x[i] & m, z = x[i] | ~m;
        sum = __builtin_amdgcn_sad_u8(y, 0u, sum);
        c20 += __popc(qual_ge(x[i], 33 + 20) & m);
        c30 += __popc(qual_ge(x[i], 33 + 30) & m);
        mn0 = qual_pk_min(mn0, z & 0x00FF00FFu); mn1 = qual_pk_min(mn1, (z >> 8) & 0x00FF00FFu);
        mx0 = qual_pk_max(mx0, y & 0x00FF00FFu); mx1 = qual_pk_max(mx1, (y >> 8) & 0x00FF00FFu);
    }
#pragma unroll
    for (int j = 0; j < 64; j++)
        if (FULL || (j >= a && j < b)) ee += etab[(x[j >> 2] >> (8 * (j & 3))) & 0xFFu];
    const u32 mn = qual_pk_min(mn0, mn1), mx = qual_pk_max(mx0, mx1);
    const u32 lo = mn & 0xFFFFu, lo2 = mn >> 16, hi = mx & 0xFFFFu, hi2 = mx >> 16;
    S.n += (u32)(b - a); S.sum += sum; S.q20 += c20; S.q30 += c30; S.ee += ee;
    S.mn = min(S.mn, min(lo, lo2)); S.mx = max(S.mx, max(hi, hi2));
}

// a global row (8-byte aligned) += S; with_n: its n too (record rows carry their length from the start)
__device__ __forceinline__ void qual_row_add(u64 *row, const QStat &S, bool with_n)
{
    if (!S.n) return;
    unsigned long long *o = (unsigned long long *)row;
    if (with_n) atomicAdd(o + 1, (unsigned long long)S.n);
    if (S.sum) atomicAdd(o + 2, (unsigned long long)S.sum);
    if (S.ee) atomicAdd(o + 3, (unsigned long long)S.ee);
    if (S.q20) atomicAdd(o + 4, (unsigned long long)S.q20);
    if (S.q30) atomicAdd(o + 5, (unsigned long long)S.q30);
    atomicMin((u32 *)(row + 6), S.mn); atomicMax((u32 *)(row + 6) + 1, S.mx);
}
// bin k += S: the workgroup's table for k < K, the global cycle rows behind it
__device__ __forceinline__ void qual_bin_add(QBin *bins, u32 K, u64 *cyc, u64 k, const QStat &S)
{
    if (!S.n) return;
    if (k < K) {
        QBin *b = bins + k;
        atomicAdd(&b->ns, ((unsigned long long)S.n << 32) | S.sum);
        if (S.q20) atomicAdd(&b->qq, ((unsigned long long)S.q30 << 32) | S.q20);
        if (S.ee) atomicAdd(&b->ee, (unsigned long long)S.ee);
        if (S.mn < b->mn) atomicMin(&b->mn, S.mn);
        if (S.mx > b->mx) atomicMax(&b->mx, S.mx);
    } else qual_row_add(cyc + k * QUAL_ROW_U64, S, true);
}

__device__ __forceinline__ u32 qual_down(u32 v, int d) { return (u32)__shfl_down((int)v, d); }
// Lanes with `pend` and the same key as their neighbour form a segment; S of a segment's first lane becomes the segment's sum.  Returns
// whether this lane is such a first lane.  Every lane of the wave calls it.
__device__ __forceinline__ bool qual_seg_reduce(bool pend, u64 key, QStat &S)
{
    const int lane = (int)(threadIdx.x & 63u);
    const u64 pk = shfl_u64(key, lane ? lane - 1 : 0);
    const bool pp = __shfl((int)pend, lane ? lane - 1 : 0) != 0;
    const bool head = pend && (lane == 0 || !pp || pk != key);
    const int len = seg_len(lane, head || !pend);                                 // (a segment begins at every lane that is no continuation of the lane in front of it)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 n = qual_down(S.n, d), sum = qual_down(S.sum, d), q20 = qual_down(S.q20, d), q30 = qual_down(S.q30, d), mn = qual_down(S.mn, d), mx = qual_down(S.mx, d);
        const u32 e0 = qual_down((u32)S.ee, d), e1 = qual_down((u32)(S.ee >> 32), d);
        if (d < len) { S.n += n; S.sum += sum; S.q20 += q20; S.q30 += q30; S.mn = min(S.mn, mn); S.mx = max(S.mx, mx); S.ee += ((u64)e1 << 32) | e0; }
    }
    return head;
}

struct QualP {
    const u8 *q; u64 b_lo, b_hi;               // pointer to byte 0 of the quality stream; bytes [b_lo, b_hi) of it may be read
    const u64 *rec_base;                       // records [r_lo, r_hi) are counted: rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi
    u64 r_lo, r_hi, p_lo, p_hi;
    u64 t0, ntiles;                            // first byte of tile 0 (b_lo <= t0 <= p_lo), tiles that reach p_hi
    u64 W;                                     // bin width of the cycle table, 0: none
    u32 K;                                     // bins kept in LDS: min(QUAL_LDS_BINS, cycle rows)
    u32 flush_iters;                           // rounds of 4 tiles between two flushes of a workgroup's LDS tables, 1 .. QUAL_FLUSH_ITERS
    u64 *rec_rows;                             // row of record r_lo (7 u64 a row, 8-byte aligned, initialised), null: not wanted
    u64 *cyc_rows;                             // cycle row 0, initialised; not null when W
    unsigned long long *hist;                  // 256 counts, null: not wanted
    u64 *total;                                // the total row, initialised
};

__global__ __launch_bounds__(256) void k_qual_count(QualP P)
{
    __shared__ u64 etab[256];
    __shared__ u32 hist[4][256];
    __shared__ QBin bins[QUAL_LDS_BINS];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    etab[tid] = qual_err_of(qual_err_33_dev, tid);
    for (u32 i = 0; i < 4; i++) hist[i][tid] = 0;
    for (u32 k = tid; k < P.K; k += 256) { bins[k].ns = 0; bins[k].qq = 0; bins[k].ee = 0; bins[k].mn = 255; bins[k].mx = 0; }
    __syncthreads();

    auto flush = [&]() {                                                          // between two barriers
        for (u32 k = tid; k < P.K; k += 256) {
            QBin &b = bins[k];
            if (!b.ns) continue;
            QStat S; S.n = (u32)(b.ns >> 32); S.sum = (u32)b.ns; S.q20 = (u32)b.qq; S.q30 = (u32)(b.qq >> 32); S.ee = b.ee; S.mn = b.mn; S.mx = b.mx;
            qual_row_add(P.cyc_rows + (u64)k * QUAL_ROW_U64, S, true);
            b.ns = 0; b.qq = 0; b.ee = 0; b.mn = 255; b.mx = 0;
        }
        if (P.hist) {
            const u32 v = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
            if (v) atomicAdd(&P.hist[tid], (unsigned long long)v);
            for (u32 i = 0; i < 4; i++) hist[i][tid] = 0;
        }
    };

    u64 Tn = 0, Tsum = 0, Tee = 0, T20 = 0, T30 = 0; u32 Tmn = 255, Tmx = 0;      // the lane's share of the total
    const u64 stride = (u64)gridDim.x * 4, iters = (P.ntiles + stride - 1) / stride, W = P.W;
    u32 *myhist = hist[wave];
    for (u64 it = 0; it < iters; it++) {
        const u64 tile = it * stride + (u64)xcd_block() * 4 + wave;
        if (tile < P.ntiles) {                                                    // (the same for all lanes of a wave)
            const u64 g = P.t0 + tile * QUAL_TILE + lane * 64;                    // the lane's first byte
            const u64 lo = g > P.p_lo ? g : P.p_lo, hi = g + 64 < P.p_hi ? g + 64 : P.p_hi;   // the bytes of it that are counted
            const bool active = lo < hi;
            u32 x[16];
#pragma unroll
            for (int i = 0; i < 16; i++) x[i] = 0;
            if (active) {
                if (g >= P.b_lo && g + 64 <= P.b_hi) {
#pragma unroll
                    for (int i = 0; i < 4; i++) { u32x4 v; memcpy(&v, P.q + g + 16 * i, 16); x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w; }
                } else {                                                          // the head or the tail of what was decoded
#pragma unroll
                    for (int j = 0; j < 64; j++) if (g + j >= lo && g + j < hi) x[j >> 2] |= (u32)P.q[g + j] << (8 * (j & 3));
                }
                if (P.hist) {
                    const int a0 = (int)(lo - g), b0 = (int)(hi - g);
#pragma unroll
                    for (int j = 0; j < 64; j++) if (j >= a0 && j < b0) atomicAdd(&myhist[(x[j >> 2] >> (8 * (j & 3))) & 0xFFu], 1u);
                }
            }
            bool pr = false, pc = false; u64 krec = 0, kcyc = 0;                  // the lane is one part (of one bin): kept for the wave's sums
            QStat PS; qual_zero(PS);
            if (active) {
                u64 r = upper_bound_u64(P.rec_base, P.r_lo, P.r_hi + 1, lo) - 1;  // rec_base[r] <= lo < rec_base[r + 1]
                u64 rbase = P.rec_base[r], rend = P.rec_base[r + 1];
                u64 at = lo;
                for (;;) {
                    const u64 e = hi < rend ? hi : rend;
                    const int a = (int)(at - g), b = (int)(e - g);
                    const bool full = a == 0 && b == 64;
                    // (left alone, the compiler takes the 64 bytes apart in front of the loop and keeps them; opaque, every part does its own)
#pragma unroll
                    for (int i = 0; i < 16; i++) asm volatile("" : "+v"(x[i]));
                    QStat S; qual_zero(S);
                    u64 k0 = 0, rem = 0; bool single = true;
                    if (W) {
                        const u64 pos = at - rbase;                               // the part's first position in its read
                        if (W == 1) k0 = pos;
                        else if (((pos | W) >> 32) == 0) { k0 = (u32)pos / (u32)W; rem = (u32)pos % (u32)W; }
                        else { k0 = pos / W; rem = pos % W; }
                        single = W - rem >= (u64)(b - a);
                    }
                    if (W && !single && W < QUAL_SMALL_W) {                       // byte by byte: S, and a bin whenever one is complete
                        QStat B; qual_zero(B);
                        u64 k = k0; u32 left = (u32)(W - rem);                    // bytes until the bin ends
#pragma unroll
                        for (int j = 0; j < 64; j++) {
                            if (j >= a && j < b) {
                                const u32 v = (x[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                                B.n++; B.sum += v; B.q20 += v >= 33 + 20; B.q30 += v >= 33 + 30; B.mn = min(B.mn, v); B.mx = max(B.mx, v); B.ee += etab[v];
                                if (--left == 0 || j == b - 1) {
                                    qual_bin_add(bins, P.K, P.cyc_rows, k, B);
                                    S.n += B.n; S.sum += B.sum; S.q20 += B.q20; S.q30 += B.q30; S.mn = min(S.mn, B.mn); S.mx = max(S.mx, B.mx); S.ee += B.ee;
                                    qual_zero(B); k++; left = (u32)W;
                                }
                            }
                        }
                    } else {
                        if (full) qual_span<true>(x, 0, 64, etab, S); else qual_span<false>(x, a, b, etab, S);
                        if (W) {
                            if (single) { if (full) { pc = true; kcyc = k0; } else qual_bin_add(bins, P.K, P.cyc_rows, k0, S); }
                            else {                                                // bin by bin under byte masks
                                int sa = a; u64 k = k0, room = W - rem;
                                while (sa < b) {
                                    const int sb = room < (u64)(b - sa) ? sa + (int)room : b;
#pragma unroll
                                    for (int i = 0; i < 16; i++) asm volatile("" : "+v"(x[i]));
                                    QStat B; qual_zero(B);
                                    qual_span<false>(x, sa, sb, etab, B);
                                    qual_bin_add(bins, P.K, P.cyc_rows, k, B);
                                    sa = sb; k++; room = W;
                                }
                            }
                        }
                    }
                    if (P.rec_rows) { if (full) { pr = true; krec = r - P.r_lo; } else qual_row_add(P.rec_rows + (r - P.r_lo) * QUAL_ROW_U64, S, false); }
                    Tn += S.n; Tsum += S.sum; Tee += S.ee; T20 += S.q20; T30 += S.q30; Tmn = min(Tmn, S.mn); Tmx = max(Tmx, S.mx);
                    if (full) PS = S;
                    at = e;
                    if (at >= hi) break;
                    do { r++; rbase = rend; rend = P.rec_base[r + 1]; } while (rend <= at);     // the next record that has bytes (at < hi <= p_hi: there is one)
                }
            }
            if (__ballot(pr)) {                                                   // whole lanes of one record: one lane adds their sum
                QStat R = PS;
                if (qual_seg_reduce(pr, krec, R)) qual_row_add(P.rec_rows + krec * QUAL_ROW_U64, R, false);
            }
            if (__ballot(pc)) {                                                   // whole lanes of one bin (neighbouring records share bin 0)
                QStat R = PS;
                if (qual_seg_reduce(pc, kcyc, R)) qual_bin_add(bins, P.K, P.cyc_rows, kcyc, R);
            }
        }
        if ((it + 1) % P.flush_iters == 0 && it + 1 < iters) { __syncthreads(); flush(); __syncthreads(); }
    }
    __syncthreads();
    flush();
    // the total: the lanes' shares, summed across the wave
    for (int d = 32; d; d >>= 1) {
        const int o = (int)(lane ^ (u32)d);
        Tn += shfl_u64(Tn, o); Tsum += shfl_u64(Tsum, o); Tee += shfl_u64(Tee, o); T20 += shfl_u64(T20, o); T30 += shfl_u64(T30, o);
        Tmn = min(Tmn, (u32)__shfl((int)Tmn, o)); Tmx = max(Tmx, (u32)__shfl((int)Tmx, o));
    }
    if (lane == 0 && Tn) {
        unsigned long long *o = (unsigned long long *)P.total;
        atomicAdd(o + 1, (unsigned long long)Tn); atomicAdd(o + 2, (unsigned long long)Tsum); atomicAdd(o + 3, (unsigned long long)Tee);
        atomicAdd(o + 4, (unsigned long long)T20); atomicAdd(o + 5, (unsigned long long)T30);
        atomicMin((u32 *)(P.total + 6), Tmn); atomicMax((u32 *)(P.total + 6) + 1, Tmx);
    }
}

// rows[j] = { key0 + j, len ? len[j] : 0, 0, 0, 0, 0, min 255 | max 0 }, j < n
__global__ __launch_bounds__(256) void k_qual_rows(u64 *rows, u64 n, u64 key0, const u64 *len)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    u64 *o = rows + j * QUAL_ROW_U64;
    o[0] = key0 + j; o[1] = len ? len[j] : 0; o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 255;
}
// *out = max(*out, the longest of len[0 .. n))
__global__ __launch_bounds__(256) void k_qual_maxlen(const u64 *len, u64 n, unsigned long long *out)
{
    u64 m = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) m = len[i] > m ? len[i] : m;
    m = wave_max_u64(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, (unsigned long long)m);
}
// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int naf_gpu_quality_error_table(uint64_t tab[256])
{
    if (!tab) return NAF_GPU_EARG;
    for (u32 b = 0; b < 256; b++) tab[b] = qual_err_of(qual_err_33, b);
    return 0;
}

// records_front for a call on the quality stream -- the record tables from the lengths alone, any sequence type; neither sequence nor
// mask nor ids are decoded -- and the check that every base has its quality code.
static int quality_front(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, u64 first, u64 *count, UnnafPlan &pl)
{
    int rc = records_front(c, d_naf, naf_len, FRONT_QUALITY, "quality", nullptr, first, count, pl);
    if (rc || !*count) return rc;
    const naf_gpu_header &h = pl.h;
    u64 bases = 0;
    if ((rc = ctx_readback(c, &bases, pl.P.rec_base + h.n_sequences, 8))) return rc;
    if (h.orig_size[S_QUAL] < bases)
        return ctx_fail(c, NAF_GPU_EFORMAT, "corrupted quality: %llu quality codes stored for %llu bases\n", (unsigned long long)h.orig_size[S_QUAL], (unsigned long long)bases);
    return 0;
}

static int quality_run(naf_gpu_ctx *c, const u8 *d_naf, size_t naf_len, u64 W, u64 first, u64 count, u8 *d_rec, size_t rec_cap, u8 *d_cyc, size_t cyc_cap,
                       u64 *n_records, u64 *n_cycle_rows, u64 *h_hist, naf_gpu_qual_row *h_total, bool rows_only)
{
    if (!c || !d_naf || !n_records || !n_cycle_rows) return NAF_GPU_EARG;
    *n_records = *n_cycle_rows = 0;
    if (h_hist) memset(h_hist, 0, 256 * sizeof *h_hist);
    if (h_total) { memset(h_total, 0, sizeof *h_total); h_total->min = 255; }
    UnnafPlan pl;
    int rc = quality_front(c, d_naf, naf_len, first, &count, pl);
    if (rc || !count) return rc;
    const EmitP &P = pl.P;
    *n_records = count;

    // the longest selected record: the cycle table's rows
    LAUNCH_LIMIT(c, count, 1, "quality: %llu records are too many for one launch", (unsigned long long)count);
    u64 *d_sum = arena_new<u64>(c, 8 + 256); if (!d_sum) return NAF_GPU_ENOMEM;   // [0] longest, [1..7] the total row, [8..263] the histogram
    HIP_TRY(c, hipMemsetAsync(d_sum, 0, (8 + 256) * 8, c->stream));
    u64 maxlen = 0;
    if (W) {
        const u64 nb = (count + 255) / 256;
        LAUNCH(c, "unnaf_qual_maxlen", k_qual_maxlen, (u32)(nb < 1024 ? nb : 1024), 256, 0, P.rec_len + first, count, (unsigned long long *)d_sum);
        if ((rc = ctx_readback(c, &maxlen, d_sum, 8))) return rc;
    }
    const u64 C = W ? maxlen / W + (maxlen % W != 0) : 0;
    *n_cycle_rows = C;
    if (rows_only) return 0;
    const bool want_rec = d_rec != nullptr, want_cyc = W && d_cyc;
    if ((want_rec && count > rec_cap) || (want_cyc && C > cyc_cap))
        return ctx_fail(c, NAF_GPU_ECAP, "quality: %llu record rows, capacity %zu; %llu cycle rows, capacity %zu", (unsigned long long)count, want_rec ? rec_cap : (size_t)0,
                        (unsigned long long)C, want_cyc ? cyc_cap : (size_t)0);
    std::vector<RecPiece> pieces;
    if ((rc = piece_plan(c, P, first, count, "QUALITY_PIECE", QUAL_PIECE_DEFAULT, pieces))) return rc;
    if (h_total) h_total->key = count;

    u64 *d_total = d_sum + 1, *d_cyc_acc = nullptr;
    LAUNCH(c, "unnaf_qual_rows", k_qual_rows, 1, 256, 0, d_total, (u64)1, count, (const u64 *)nullptr);
    if (want_cyc && C) {
        LAUNCH_LIMIT(c, C, QUAL_ROW_U64, "quality: %llu cycle rows are too many for one launch", (unsigned long long)C);
        d_cyc_acc = arena_new<u64>(c, C * QUAL_ROW_U64); if (!d_cyc_acc) return NAF_GPU_ENOMEM;
        LAUNCH(c, "unnaf_qual_rows", k_qual_rows, (u32)((C + 255) / 256), 256, 0, d_cyc_acc, C, (u64)0, (const u64 *)nullptr);
    }
    const u32 K = d_cyc_acc ? (u32)(C < QUAL_LDS_BINS ? C : QUAL_LDS_BINS) : 0u;
    int cus = 0;
    HIP_TRY(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    u64 max_grid = (u64)(cus > 0 ? cus : 1) * QUAL_WG_PER_CU;
    u32 flush_iters = QUAL_FLUSH_ITERS;                                          // the levers can only make the grid smaller and the flushes more frequent
    { const char *e = ctx_opt(c, "QUALITY_GRID"); if (e && e[0]) { const u64 v = strtoull(e, nullptr, 10); if (v && v < max_grid) max_grid = v; } }
    { const char *e = ctx_opt(c, "QUALITY_FLUSH"); if (e && e[0]) { const u64 v = strtoull(e, nullptr, 10); if (v && v < flush_iters) flush_iters = (u32)v; } }
    const u64 q_bytes = pl.h.orig_size[S_QUAL];

    PieceSweep sw(c, d_naf, pl, "quality", S_QUAL);
    for (size_t pi = 0; pi < pieces.size(); pi++) {
        const RecPiece &pc = pieces[pi];
        const u64 nr = pc.r_hi - pc.r_lo;
        LAUNCH_LIMIT(c, nr, QUAL_ROW_U64, "quality: a piece of %llu records is too long for one launch", (unsigned long long)nr);
        QualP Q; memset(&Q, 0, sizeof Q);
        if (pc.p_hi > pc.p_lo) {
            PayloadSpan sp;
            if ((rc = sw.bytes_for(pc.p_lo, pc.p_hi, &sp))) return rc;
            Q.q = sp.base; Q.b_lo = sp.got_lo; Q.b_hi = sp.got_hi;
            if (Q.b_lo > pc.p_lo || Q.b_hi < pc.p_hi) return ctx_fail(c, NAF_GPU_EFORMAT, "can't decompress quality\n");
        }
        u64 *acc = nullptr;
        if (want_rec) {
            acc = arena_new<u64>(c, nr * QUAL_ROW_U64); if (!acc) return NAF_GPU_ENOMEM;
            LAUNCH(c, "unnaf_qual_rows", k_qual_rows, (u32)((nr + 255) / 256), 256, 0, acc, nr, pc.r_lo, P.rec_len + pc.r_lo);
        }
        if (pc.p_hi > pc.p_lo) {
            const u64 mis = (u64)((uintptr_t)(Q.q + pc.p_lo) & 15u);              // tiles start on a 16-byte address when the decoded range reaches that far down
            Q.t0 = pc.p_lo - Q.b_lo >= mis ? pc.p_lo - mis : pc.p_lo;
            Q.ntiles = (pc.p_hi - Q.t0 + QUAL_TILE - 1) / QUAL_TILE;
            Q.rec_base = P.rec_base; Q.r_lo = pc.r_lo; Q.r_hi = pc.r_hi; Q.p_lo = pc.p_lo; Q.p_hi = pc.p_hi;
            Q.W = d_cyc_acc ? W : 0; Q.K = K; Q.flush_iters = flush_iters; Q.rec_rows = acc; Q.cyc_rows = d_cyc_acc;
            Q.hist = h_hist ? (unsigned long long *)d_sum + 8 : (unsigned long long *)nullptr; Q.total = d_total;
            const u64 wgs = (Q.ntiles + 3) / 4;
            LAUNCH(c, "unnaf_qual_count", k_qual_count, (u32)(wgs < max_grid ? wgs : max_grid), 256, 0, Q);
        }
        if (want_rec) rows_copy(c, "unnaf_row_copy", acc, d_rec + 56 * (pc.r_lo - first), nr, QUAL_ROW_U64);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        sw.release();
    }
    if (d_cyc_acc) rows_copy(c, "unnaf_row_copy", d_cyc_acc, d_cyc, C, QUAL_ROW_U64);
    HIP_TRY(c, hipGetLastError());
    u64 sum[8 + 256];
    if ((rc = ctx_readback(c, sum, d_sum, sizeof sum))) return rc;                // (waits for the copy too)
    if (h_hist) memcpy(h_hist, sum + 8, 256 * 8);
    if (h_total) { h_total->n = sum[2]; h_total->sum = sum[3]; h_total->ee = sum[4]; h_total->n_q20 = sum[5]; h_total->n_q30 = sum[6]; h_total->min = (u32)sum[7]; h_total->max = (u32)(sum[7] >> 32); }
    if (ctx_tracing(c)) ctx_trace(c, "[quality] records %llu cycle rows %llu pieces %zu quality bytes decoded %llu of %llu lds bins %u global bins %llu\n", (unsigned long long)count,
                                  (unsigned long long)C, pieces.size(), (unsigned long long)sw.decoded, (unsigned long long)q_bytes, K, (unsigned long long)(d_cyc_acc ? C - K : 0));
    return 0;
}

extern "C" int naf_gpu_unnaf_quality_rows(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t cycle_bin, uint64_t first, uint64_t count,
                                          uint64_t *n_records, uint64_t *n_cycle_rows)
{
    int rc = quality_run(c, (const u8 *)d_naf, naf_len, cycle_bin, first, count, nullptr, 0, nullptr, 0, n_records, n_cycle_rows, nullptr, nullptr, true);
    if (c) arena_settle(c);
    return rc;
}
extern "C" int naf_gpu_unnaf_quality(naf_gpu_ctx *c, const void *d_naf, size_t naf_len, uint64_t cycle_bin, uint64_t first, uint64_t count,
                                     naf_gpu_qual_row *d_rec_rows, size_t rec_cap, naf_gpu_qual_row *d_cycle_rows, size_t cycle_cap,
                                     uint64_t *n_records, uint64_t *n_cycle_rows, uint64_t h_hist[256], naf_gpu_qual_row *h_total)
{
    int rc = quality_run(c, (const u8 *)d_naf, naf_len, cycle_bin, first, count, (u8 *)d_rec_rows, rec_cap, (u8 *)d_cycle_rows, cycle_cap, n_records, n_cycle_rows,
                         h_hist, h_total, false);
    if (c) arena_settle(c);
    return rc;
}
