// reads.h -- what the read filters share (trim.h, clip.h, dedup.h, screen.h; the segment length serves quality.h too).  Part of emit.hip
// (included by it, in front of quality.h).  The lane loads are packed.h's, the wave sums wgscan.h's, the host's pieces, levers and row
// tables payload.h's.
//   k_bounds_stage   the caller's bounds rows -> windows, carried flags, "takes part", the first row that is none
//   bounds_row_fail  the host's message for that row
//   wg_sums          the lanes' counters -> one atomic per non-zero counter and workgroup
//   lane_parts       a lane's bytes or bases, record by record
//   seam_carry       the parts of one record across the lanes of a wavefront -> the summary of its bytes in the tile
//   seam_join        the summaries of one record across tiles (two slots a tile) -> the record's
//   ReadsPiece       a piece of the packed stream as a kernel sees it
#pragma once

#define BOUNDS_OK 0xFFFFFFFFFFFFFFFFull          // *bad when every bounds row is one

// A lane per selected record.  bounds: the caller's rows (`stride` bytes each, any alignment: record, begin, end as u64 at bytes 0, 8, 16,
// the flags word at byte flags_at), null: the whole records, whose flags are NAF_GPU_TRIM_KEPT.  win[2k], win[2k + 1]: the window of record
// first + k, inside the record whatever the row said, so that no kernel behind this one depends on the caller's numbers; wflags[k]: the
// flags under keep_mask; part[k] (null: not wanted): NAF_GPU_TRIM_KEPT is among them.  *bad (preset to BOUNDS_OK): k << 2 | what of the
// first row that is none (1: its record, 2: begin > end, 3: end > the record's length), the smallest by atomicMin.  (No counter here: one
// atomic a wavefront on a single counter took 7.2 ms for 38 M records, the kernel without it 0.20 ms.)
__global__ __launch_bounds__(256) void k_bounds_stage(const u8 *bounds, u32 stride, u32 flags_at, u32 keep_mask, const u64 *rec_base, u64 first, u64 count,
                                                      u64 *win, u32 *wflags, u8 *part, unsigned long long *bad)
{
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const u64 n = rec_base[first + k + 1] - rec_base[first + k];
    u64 b = 0, e = n; u32 f = NAF_GPU_TRIM_KEPT;
    if (bounds) {
        const u8 *p = bounds + (u64)stride * k;
        const u64 rec = ld64(p);
        b = ld64(p + 8); e = ld64(p + 16); f = ld32(p + flags_at);
        const u32 what = rec != first + k ? 1u : b > e ? 2u : e > n ? 3u : 0u;
        if (what) atomicMin(bad, (unsigned long long)(k << 2 | what));
        if (e > n) e = n;
        if (b > e) b = e;
    }
    f &= keep_mask;
    win[2 * k] = b; win[2 * k + 1] = e; wflags[k] = f;
    if (part) part[k] = (f & NAF_GPU_TRIM_KEPT) != 0;
}

// bad: what k_bounds_stage left, not BOUNDS_OK
static int bounds_row_fail(naf_gpu_ctx *c, const char *who, u64 bad)
{
    const u32 what = (u32)(bad & 3);
    return ctx_fail(c, NAF_GPU_EARG, "%s: bounds row %llu: %s", who, (unsigned long long)(bad >> 2),
                    what == 1 ? "its record is not first + its number (one row per selected record, ascending)" : what == 2 ? "begin > end" : "end is behind the record's last base");
}

// The lanes' counters T: combined across the wavefront, then across the workgroup in lds[N] (zeroed behind a barrier by the caller), then
// into total[N], one atomic per non-zero counter and workgroup.  Bit k of MAX: counter k is a maximum, not a sum.  Integers, so the
// totals do not depend on the order.  Every lane of the workgroup calls it.
template <u32 N, u32 MAX = 0>
__device__ __forceinline__ void wg_sums(const u64 (&T)[N], unsigned long long *lds, unsigned long long *total)
{
    const u32 lane = threadIdx.x & 63u;
#pragma unroll
    for (u32 k = 0; k < N; k++) {
        const bool mx = (MAX >> k) & 1u;
        const u64 v = mx ? wave_max_u64(T[k]) : wave_sum_u64(T[k]);
        if (lane == 0 && v) { if (mx) atomicMax(&lds[k], (unsigned long long)v); else atomicAdd(&lds[k], (unsigned long long)v); }
    }
    __syncthreads();
    if (threadIdx.x < N && lds[threadIdx.x]) { if ((MAX >> threadIdx.x) & 1u) atomicMax(&total[threadIdx.x], lds[threadIdx.x]); else atomicAdd(&total[threadIdx.x], lds[threadIdx.x]); }
}

// The lane's positions [lo, hi) (lo < hi) of a stream whose records [r_lo, r_hi) lie at rec_base (p_lo = rec_base[r_lo] <= lo,
// hi <= rec_base[r_hi] = p_hi), part by part -- a part: the lane's positions of one record --: body(r, rbase, rend, at, stop) for positions
// [at, stop) of record r = [rbase, rend).  The first record by one upper_bound, the others by walking on; records without positions get
// no call.
template <typename Body>
__device__ __forceinline__ void lane_parts(const u64 *rec_base, u64 r_lo, u64 r_hi, u64 lo, u64 hi, Body body)
{
    u64 r = upper_bound_u64(rec_base, r_lo, r_hi + 1, lo) - 1;                    // rec_base[r] <= lo < rec_base[r + 1]
    u64 rbase = rec_base[r], rend = rec_base[r + 1], at = lo;
    for (;;) {
        const u64 stop = rend < hi ? rend : hi;
        body(r, rbase, rend, at, stop);
        if (stop >= hi) break;
        at = stop;
        do { r++; rbase = rend; rend = rec_base[r + 1]; } while (rend <= at);    // the next record that has positions (at < hi <= p_hi: there is one)
    }
}

// Lanes with `first` begin a segment; returns the lanes [lane, lane + len) from this one to its segment's last.  Every lane of the wave calls it.
__device__ __forceinline__ int seg_len(int lane, bool first)
{
    const u64 cut = __ballot(first);
    const u64 above = lane == 63 ? 0ull : cut >> (lane + 1);
    return above ? __ffsll((long long)above) : 64 - lane;
}

// A lane's parts of records that do not end in it, as summaries S of an associative combine(L, R) (L's bytes, then R's): A (has_a) ends a
// record of the lane in front, X (pend) is of a record that goes on in the next lane, thru: X came from the lane in front too.  Every A
// moves one lane down into the X in front of it (the byte in front of it is that lane's last and the same record's; lane 0's A came from
// the tile in front and stays the caller's), and the X of one record -- its first lane here, then through-parts -- are combined in lane
// order by a segmented reduction of log steps.  down(S, d): lane + d's S.  Returns whether the lane is the first of its record here: its X
// is then the summary of all the record has in the wavefront's tile.  Every lane of the wave calls it.
template <typename S, typename Down, typename Combine>
__device__ __forceinline__ bool seam_carry(u32 lane, bool has_a, const S &A, bool pend, bool thru, S &X, Down down, Combine combine)
{
    if (!__ballot(pend || has_a)) return false;
    const S N = down(A, 1);
    const bool na = __shfl_down((int)has_a, 1) != 0 && lane < 63;
    if (na && pend) X = combine(X, N);
    const bool head = pend && (!thru || lane == 0);
    const int len = seg_len((int)lane, head || !pend);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const S Y = down(X, d);
        if (pend && d < len) X = combine(X, Y);
    }
    return head;
}

// Record [rbase, rend) (rend > rbase) in tiles of `tile` positions from t0 on, whose slots are open[2 t] (a record that began in front of
// tile t) and open[2 t + 1] (one that begins in it and ends behind it).  Which slot a record's part of a tile went to follows from the
// positions alone, so no slot needs a mark.  Returns the tiles the record touches; more than one: out = slot 1 of the first combined with
// slot 0 of every later one, in tile order.  One step a tile.
template <typename S, typename Combine>
__device__ __forceinline__ u64 seam_join(const S *open, u64 t0, u32 tile, u64 rbase, u64 rend, S &out, Combine combine)
{
    const u64 a = (rbase - t0) / tile, b = (rend - 1 - t0) / tile;
    if (b > a) {
        out = open[2 * a + 1];
        for (u64 t = a + 1; t <= b; t++) out = combine(out, open[2 * t]);
    }
    return b - a + 1;
}

// A piece of the packed stream under a kernel.  seq: pointer to packed byte 0 of the stream; bytes [.., b_end) of it may be read.
// Records [r_lo, r_hi): rec_base[r_lo] = p_lo, rec_base[r_hi] = p_hi.  t0: first base of tile 0 (even, <= p_lo); ntiles reach p_hi.
struct ReadsPiece {
    const u8 *seq; u64 b_end;
    const u64 *rec_base;
    u64 r_lo, r_hi, p_lo, p_hi;
    u64 t0, ntiles;
    ReadsPiece() = default;
    // tl: what PieceSweep::seq_for gave for pc; all zero for a piece without bases
    ReadsPiece(const EmitP &P, const RecPiece &pc, const PieceSweep::Tiles &tl)
        : seq(tl.seq), b_end(tl.b_hi), rec_base(P.rec_base), r_lo(pc.r_lo), r_hi(pc.r_hi), p_lo(pc.p_lo), p_hi(pc.p_hi), t0(tl.t0), ntiles(tl.ntiles) {}
};
