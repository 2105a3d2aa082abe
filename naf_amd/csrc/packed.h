// packed.h -- what the kernels that scan the packed 4-bit stream share on the device (locate.h, composition.h, runs.h, kmers.h; the row copy
// serves quality.h too).  Part of emit.hip (included by it at its top); the host parts these callers share are payload.h's.
// A tile starts on an even base, so a lane's first base g is the low nibble of byte g >> 1 (the first base of a byte is its low nibble),
// and base j of a lane is nibble j & 7 of dword j >> 3.  packed_tail is the ONLY loop that reads next to the stream's end.
#pragma once
#include "common.h"

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
#define NIB_L 0x11111111u

// w[k] = bytes [b0 + sizeof(T) k, b0 + sizeof(T) (k + 1)) of seq, k < N, little endian; a byte at or behind b_end is not touched and reads as 0
template <u32 N, typename T>
__device__ __forceinline__ void packed_tail(const u8 *seq, u64 b_end, u64 b0, T *w)
{
    const u32 B = (u32)sizeof(T);
#pragma unroll
    for (u32 k = 0; k < N; k++) {
        T v = 0;
        for (u32 i = 0; i < B; i++) if (b0 + B * k + i < b_end) v |= (T)seq[b0 + B * k + i] << (8 * i);
        w[k] = v;
    }
}

// x = the 64 bases from base g on (g even): two 16-byte loads of any alignment where all 32 bytes lie in front of b_end, else byte by byte.
// seq: pointer to packed byte 0 of the stream; bytes [.., b_end) of it may be read.
__device__ __forceinline__ void packed_load64(const u8 *seq, u64 b_end, u64 g, u32 (&x)[8])
{
    const u64 b0 = g >> 1;
    if (b0 + 32 > b_end) return packed_tail<8>(seq, b_end, b0, x);
    u32x4 v0, v1; memcpy(&v0, seq + b0, 16); memcpy(&v1, seq + b0 + 16, 16);
    x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
}

// The code of the base behind a lane's 64 (0 where there is none to read).  Every lane of the wave calls it (one shuffle): x = what
// packed_load64 gave it, zeros in a lane that is not `active`; lane 63 reads byte (g >> 1) + 32 when that lies in front of b_end.
__device__ __forceinline__ u32 packed_behind(const u8 *seq, u64 b_end, u64 g, bool active, u32 lane, const u32 (&x)[8])
{
    u32 nc = 0;
    if (active && lane == 63 && (g >> 1) + 32 < b_end) nc = seq[(g >> 1) + 32];
    const u32 dn = (u32)__shfl_down((int)x[0], 1);
    return (lane != 63 ? dn : nc) & 15u;
}
// The codes of the twelve bases behind a lane's 64 as 48 bits, the nearest in the low nibble (0 where there is none to read).  Every lane of
// the wave calls it (two shuffles); lane 63 reads the six bytes from (g >> 1) + 32 on that lie in front of b_end.
__device__ __forceinline__ u64 packed_behind12(const u8 *seq, u64 b_end, u64 g, bool active, u32 lane, const u32 (&x)[8])
{
    u16 w[3] = { 0, 0, 0 };
    if (active && lane == 63) packed_tail<3>(seq, b_end, (g >> 1) + 32, w);
    const u32 d0 = (u32)__shfl_down((int)x[0], 1), d1 = (u32)__shfl_down((int)x[1], 1) & 0xFFFFu;
    return lane != 63 ? (u64)d0 | ((u64)d1 << 32) : (u64)w[0] | ((u64)w[1] << 16) | ((u64)w[2] << 32);
}
// The code of the base in front of a lane's first (0 where there is none to read); as above, lane 0 reads byte (g >> 1) - 1 when
// g > p_lo: base g - 1 >= p_lo is then one of the range, in a decoded byte.
__device__ __forceinline__ u32 packed_front(const u8 *seq, u64 p_lo, u64 g, bool active, u32 lane, const u32 (&x)[8])
{
    u32 pc = 0;
    if (active && lane == 0 && g > p_lo) pc = (u32)seq[(g >> 1) - 1] >> 4;
    const u32 up = (u32)__shfl_up((int)x[7], 1) >> 28;
    return lane != 0 ? up : pc;
}

// The four bit planes of a dword's nibbles (p_b: bit b of every nibble, in the nibble's bit 0; q_b: its complement) as two groups of
// four ANDs: nibble j of lo[l] & hi[h] is 1 where nibble j of y holds code 4 h + l
__device__ __forceinline__ void nib_products(u32 y, u32 (&lo)[4], u32 (&hi)[4])
{
    const u32 p0 = y & NIB_L, p1 = (y >> 1) & NIB_L, p2 = (y >> 2) & NIB_L, p3 = (y >> 3) & NIB_L;
    const u32 q0 = p0 ^ NIB_L, q1 = p1 ^ NIB_L, q2 = p2 ^ NIB_L, q3 = p3 ^ NIB_L;
    lo[0] = q0 & q1; lo[1] = p0 & q1; lo[2] = q0 & p1; lo[3] = p0 & p1;
    hi[0] = q2 & q3; hi[1] = p2 & q3; hi[2] = q2 & p3; hi[3] = p2 & p3;
}

// n u64 from the arena (8-byte aligned) to a table of any alignment.  bad (may be null): nothing is written unless *bad is all ones (a
// call that looks at its bounds rows' verdict only at its end: reads.h)
__global__ __launch_bounds__(256) void k_row_copy(const u64 *src, u8 *dst, u64 n, const unsigned long long *bad)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (!bad || *bad == ~0ull)) st64(dst + 8 * i, src[i]);
}
