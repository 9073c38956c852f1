// text_keys.h -- packing sort keys of consecutive suffixes from the recoded text (shared by the LSD
// passes of radix_sort.hip and the MSD partition of msd_sort.hip).
#pragma once
#include "prims.h"

namespace pss {

constexpr int TK_IPT = 16;   // suffixes per thread

// The 32 code bytes the keys of suffixes i0 .. i0+15 are packed from (i0 % 16 == 0; codes are zero padded past n).
// Load and packing are separate so that a kernel can issue the load of its next tile early (msd_scatter2_kernel).
__device__ __forceinline__ void text_keys16_load(const u8 *codes, u32 i0, uint4 &lo, uint4 &hi)
{
    const uint4 *p = reinterpret_cast<const uint4 *>(codes + i0);
    lo = p[0];
    hi = p[1];
}

// Packs the keys of 16 consecutive suffixes i0 .. i0+15 from the words text_keys16_load brought.
// Sliding window: key(i+1) = ((key(i) << b) | code[i+k]) & mask.
__device__ __forceinline__ void text_keys16_pack(const uint4 &lo, const uint4 &hi, u32 i0, int b, int k, int plus_one, int drop,
                                                 u32 n, u64 (&key)[TK_IPT])
{
    const u64 q0 = (u64)lo.x | ((u64)lo.y << 32), q1 = (u64)lo.z | ((u64)lo.w << 32);
    const u64 q2 = (u64)hi.x | ((u64)hi.y << 32), q3 = (u64)hi.z | ((u64)hi.w << 32);
    const u64 mask = (k * b >= 64) ? ~0ull : ((1ull << (k * b)) - 1ull);
    // first window: bytes 0 .. k-1
    u64 win = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const u64 src = (j < 8) ? q0 : q1;
        u32 c = (u32)(src >> ((j & 7) * 8)) & 0xffu;
        if (plus_one) c = (i0 + j < n) ? c + 1u : 0u;
        if (j < k) win = (win << b) | c;
    }
    key[0] = win >> drop;
    // byte stream starting at byte k (k is wave-uniform): s0 = bytes k..k+7, s1 = k+8..k+15
    u64 a0, a1, a2;
    if (k >= 16) { a0 = q2; a1 = q3; a2 = 0; }
    else if (k >= 8) { a0 = q1; a1 = q2; a2 = q3; }
    else { a0 = q0; a1 = q1; a2 = q2; }
    const int sh = (k & 7) * 8;
    u64 s0 = a0, s1 = a1;
    if (sh) {
        s0 = (a0 >> sh) | (a1 << (64 - sh));
        s1 = (a1 >> sh) | (a2 << (64 - sh));
    }
#pragma unroll
    for (int r = 1; r < TK_IPT; ++r) {
        const int j = r - 1;
        const u64 src = (j < 8) ? s0 : s1;
        u32 c = (u32)(src >> ((j & 7) * 8)) & 0xffu;
        if (plus_one) c = ((u64)i0 + j + k < n) ? c + 1u : 0u;
        win = ((win << b) | c) & mask;
        key[r] = win >> drop;
    }
}

__device__ __forceinline__ void text_keys16(const u8 *codes, u32 i0, int b, int k, int plus_one, int drop, u32 n,
                                            u64 (&key)[TK_IPT])
{
    uint4 lo, hi;
    text_keys16_load(codes, i0, lo, hi);
    text_keys16_pack(lo, hi, i0, b, k, plus_one, drop, n, key);
}

// The key of ONE suffix: the k <= 16 symbols from text position j on, b bits each, first symbol highest (the text rounds of
// sa_build.hip, the finishing kernel of msd_sort.hip).
__device__ __forceinline__ u64 text_key_at(const u8 *codes, u32 j, int b, int k, int plus_one, u32 n)
{
    // k <= 16 symbols starting at j (codes are zero padded past n).  The address is random per lane,
    // and a scattered load costs the address unit one cycle per lane and instruction whatever its
    // width: two aligned 16-byte loads and a funnel shift instead of six 4-byte loads
    // (`words` 2^29: 78.4 -> 76.0 ms).
    const uint4 *q = reinterpret_cast<const uint4 *>(codes + (j & ~15u));
    const uint4 a = q[0], c = q[1];
    const u64 x0 = (u64)a.x | ((u64)a.y << 32), x1 = (u64)a.z | ((u64)a.w << 32);
    const u64 x2 = (u64)c.x | ((u64)c.y << 32), x3 = (u64)c.z | ((u64)c.w << 32);
    const bool up = (j & 8u) != 0;
    const u32 s8 = (j & 7u) * 8u;
    const u64 l0 = up ? x1 : x0, l1 = up ? x2 : x1, l2 = up ? x3 : x2;
    const u64 w0 = s8 ? (l0 >> s8) | (l1 << (64 - s8)) : l0;
    const u64 w1 = s8 ? (l1 >> s8) | (l2 << (64 - s8)) : l1;
    u64 key = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < k) {
            u32 v = (u32)((c < 8 ? w0 : w1) >> ((c & 7) * 8)) & 0xffu;
            if (plus_one) v = ((u64)j + c < n) ? v + 1u : 0u;
            key = (key << b) | v;
        }
    }
    return key;
}

}  // namespace pss
