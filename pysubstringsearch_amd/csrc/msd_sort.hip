// msd_sort.hip -- initial suffix sort as a hybrid MSD radix sort, for gfx950.
//
// The LSD passes of radix_sort.hip move every suffix through HBM once per 8 key bits
// (5 scatter passes + 5 histogram reads for the 40-bit key of the `lines` corpus), and a
// scatter pass is bound by where its short runs land, not by bytes.  This
// path spends TWO global partition passes and finishes inside LDS:
//
//   G1  text -> A1   partition all n suffixes by the top 10 bits of their packed key.  The
//                    element written is 8 bytes: [ remaining key bits | suffix index ], so no
//                    second plane and nothing is gathered from the text again.
//   G2  A1 -> A2     partition every G1 bucket by the next 10 key bits ("segmented": a
//                    workgroup's range never crosses a G1 bucket).  The scan of the
//                    (range, digit) counts IS the table of the 2^20 joint bucket starts.
//   L   A2 -> SA     joint buckets are at most 4096 suffixes (checked exactly, see below):
//                    consecutive buckets are packed into tiles of < 8192 elements, one
//                    workgroup sorts a tile by (bucket, remaining key bits) entirely in LDS
//                    (stable 8-bit LSD passes, the wave-ballot ranking of radix_sort.hip) and
//                    writes the suffix indices sequentially -- full lines, no scatter -- with
//                    bit 31 = "same key as my predecessor" (the contract of suffix_sort_flags).
//
// Traffic: (1 + 1 + 8) + (8 + 8 + 8) + (8 + 4) = 46 bytes per suffix instead of 86, and two
// scattered passes instead of five.
//
// Neither global pass needs a stable order (whatever order a bucket arrives in, L sorts it),
// so the per-tile ranking is one returning LDS atomic per element -- no ballots, no per-wave
// histograms -- which is what makes 1024 bins affordable: 8192-element tiles keep the runs at
// 8 elements x 8 bytes.
//
// The path needs every joint bucket to fit a tile.  That is a property of the text (high-entropy
// text: yes; natural language: no, "the " alone overflows it), known exactly after G2's
// histogram.  The caller screens with the sorted key sample it already has; when the exact
// check fails the caller falls back to the LSD path (G1 is lost, ~4 ms at n = 2^29).
//
// Round 6 -- the two digits in LSD ORDER, the second pass in ONE sweep (decoupled look-back).  The order above makes
// the second pass wait for a histogram of its own: where bucket (b, d) starts inside G1 bucket b is only known once all
// of b has been counted -- 8 n bytes read a second time (msd_hist_kernel<false>, 0.85 ms at n = 2^29).  Taken the other
// way round the passes need the two 1024-bin histograms of the TEXT only, which one pass over its n bytes gives:
//
//   H   text          counts of the second digit d per range (the first pass's offsets) and of the first digit b
//   P1  text -> A1    partition by d; the element keeps b: [ b | remaining key bits | suffix index ]
//   P2  A1 -> A2      partition by b, tiles in order: a tile lies inside one d-region, so inside every b-bucket the tiles
//                     arrive in d order and the joint buckets (b, d) come out contiguous whatever the order inside a tile
//                     (still one returning LDS atomic per element).  Where (tile, b) goes = start of b + what the tiles
//                     before it hold of b: every tile counts its own 16384 elements (it ranks them anyway), publishes
//                     the 1024 counts and adds up what its predecessors published, back to the nearest tile that has
//                     published its running total -- no second read, no table.  Tiles are handed out by an atomic ticket,
//                     so every predecessor of a waiting tile is running.  The last tile of d-region d leaves the ends of
//                     the buckets (b, d): the table of joint bucket starts falls out of the pass.
//
// The joint table only exists after P2, so P2 cannot tag an element with its bucket's number among the non-empty ones.
// The d-regions are renumbered first (msd_tiles2_kernel: the non-empty ones 0 .. D - 1 in digit order -- a digit value
// that never occurs leaves no hole), P2 tags with that number mod 64 (a constant of the tile), the plan never lets a
// local-sort tile cross a multiple of 64 joint buckets, and the local sort takes "tag - tag of the tile's first bucket"
// as the bucket's number inside its tile: one subtraction.
// Measured in isolation before it was built: tests/tools/lookback_micro.hip, profiles/r06_lookback_micro.txt.
//
// HBM-bound integer work: no MFMA anywhere by design.
#include "msd_sort.h"

#include <algorithm>
#include <type_traits>
#include <vector>

#include "prims.h"
#include "scan.h"
#include "text_keys.h"

namespace pss {

// (geometry constants, MsdRange / MsdTile / MsdTile2 and the workspace: msd_layout.h)
constexpr int MSD_WAVES = MSD_BLOCK / kWave;

struct MsdArgs {
    // text source (G1)
    const u8 *codes;
    int code_bits, key_chars, plus_one, key_drop;
    u32 n;
    int key_bits;        // K: bits of (packed key >> key_drop) that take part in the sort
    int idx_bits;        // ib: bits of a suffix index
    // G1 geometry
    u32 tiles_per_range1, num_ranges1;
    // tables
    u32 *T;              // [ranges][1024] counts, then global offsets
    u32 *J1;             // [1025] G1 bucket starts
    u32 *J;              // [2^20 + 1] joint bucket starts
    MsdRange *ranges2;   // G2 range descriptors
    u32 *seg_first;      // [1025] first G2 range of every G1 bucket
    u32 *counters;       // [0] number of G2 ranges, [1] largest joint bucket, [2] non-empty buckets, [3] tiles
    const u64 *dense;    // G2 scatter: [2^20] number of every joint bucket among the non-empty ones
    const u64 *in;
    u64 *out;
    // LSD order (round 6): the first pass partitions by the SECOND digit, the second pass is the look-back kernel
    int lsd;
    u32 *T2;             // [1024][ranges] counts of the first digit per range (only their totals are used)
    const u32 *Jb;       // [1025] starts of the first digit's buckets
    const struct MsdTile2 *tiles2;
    u32 *status;         // [tiles2][1024] look-back words
    // MsdFront: the first histogram pass recodes the raw text on its way through
    const u8 *raw;
    const u8 *lut;
    u8 *codes_out;
    u32 *bad;
};

// Pins a loaded value: the load that produced it cannot be sunk into a later branch.
__device__ __forceinline__ void keep_load(u64 &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void keep_load(uint4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// Workgroup barrier that waits for this wave's LDS traffic only: global loads issued before it (the
// prefetch of the next tile) stay in flight across it.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- tile machinery of the two global passes -----------------------------------------------------

template <bool FROM_TEXT>
__device__ __forceinline__ void msd_load_tile(const MsdArgs &a, u32 base, u32 valid, u64 (&elem)[MSD_IPT], u32 (&dig)[MSD_IPT],
                                              int shift2)
{
    const u32 tid = threadIdx.x;
    if (FROM_TEXT) {
        // 16 consecutive suffixes per thread; element = [key bits below the top 10 | index]
        const u32 i0 = base + tid * MSD_IPT;
        u64 key[MSD_IPT] = {};
        if (i0 < a.n) text_keys16(a.codes, i0, a.code_bits, a.key_chars, a.plus_one, a.key_drop, a.n, key);
        const int rest_bits = a.key_bits - MSD_D;
        const u64 rest_mask = (1ull << rest_bits) - 1ull;
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) {
            dig[r] = (u32)(key[r] >> rest_bits) & (MSD_BINS - 1u);
            elem[r] = ((key[r] & rest_mask) << a.idx_bits) | (u64)(i0 + r);
        }
    } else {
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) {
            const u32 p = r * MSD_BLOCK + tid;
            elem[r] = p < valid ? a.in[base + p] : 0ull;
            dig[r] = (u32)(elem[r] >> shift2) & (MSD_BINS - 1u);
        }
    }
}

template <bool FROM_TEXT>
__device__ __forceinline__ bool msd_valid(u32 base, u32 valid, int r, u32 n)
{
    const u32 tid = threadIdx.x;
    (void)base;
    (void)n;
    return FROM_TEXT ? (tid * MSD_IPT + r < valid) : (r * MSD_BLOCK + tid < valid);
}

template <bool FROM_TEXT>
__global__ __launch_bounds__(MSD_BLOCK) void msd_hist_kernel(MsdArgs a)
{
    __shared__ u32 hist[MSD_BINS];
    __shared__ u32 histb[FROM_TEXT ? MSD_BINS : 1];      // LSD order: the first digit, counted in the same pass
    const u32 tid = threadIdx.x, r = blockIdx.x;
    u32 e0, e1;
    if (FROM_TEXT) {
        if (r >= a.num_ranges1) return;
        e0 = r * a.tiles_per_range1 * MSD_TILE;
        const u64 end = (u64)(r + 1) * a.tiles_per_range1 * MSD_TILE;
        e1 = end < a.n ? (u32)end : a.n;
    } else {
        if (r >= a.counters[0]) return;
        e0 = a.ranges2[r].start;
        e1 = a.ranges2[r].end;
    }
    for (u32 i = tid; i < MSD_BINS; i += MSD_BLOCK) {
        hist[i] = 0;
        if (FROM_TEXT) histb[i] = 0;
    }
    __syncthreads();
    const int shift2 = a.idx_bits + a.key_bits - 2 * MSD_D;
    if (FROM_TEXT) {
        // the digit is the top 10 bits of the key: the first m = ceil(10 / b) symbols are all it takes -- a 32-bit
        // sliding window instead of the 64-bit keys of text_keys16 (0.41 -> 0.16 ms at n = 2^29).  LSD order: the top
        // 20 bits, m = ceil(20 / b) symbols (<= 24 bits), the pass's own digit is the LOWER ten of them.
        const int b = a.code_bits;
        const int top = a.lsd ? 2 * MSD_D : MSD_D;
        const int m = (top + b - 1) / b;
        const u32 wmask = (m * b >= 32) ? ~0u : ((1u << (m * b)) - 1u);
        const int down = m * b - top;
        // (the next tile's 32 bytes are loaded before this tile's atomics: two trips to HBM in flight per thread)
        uint4 nlo = make_uint4(0, 0, 0, 0), nhi = nlo;
        if (e0 + tid * MSD_IPT < e1) {
            const uint4 *p = reinterpret_cast<const uint4 *>(a.codes + e0 + tid * MSD_IPT);
            nlo = p[0];
            nhi = p[1];
        }
        for (u32 base = e0; base < e1; base += MSD_TILE) {
            const u32 i0 = base + tid * MSD_IPT;
            const uint4 lo = nlo, hi = nhi;
            if ((u64)i0 + MSD_TILE < e1) {
                const uint4 *p = reinterpret_cast<const uint4 *>(a.codes + i0 + MSD_TILE);
                nlo = p[0];
                nhi = p[1];
            }
            if (i0 >= e1) continue;
            const u64 q[4] = {(u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                              (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32)};
            auto sym = [&](u32 j) -> u32 { return (u32)(q[j >> 3] >> ((j & 7u) * 8u)) & 0xffu; };   // codes are 0 past the text
            u32 win = 0;
            for (int t = 0; t < m; ++t) win = (win << b) | sym((u32)t);
#pragma unroll
            for (int r = 0; r < MSD_IPT; ++r) {
                if (r > 0) win = ((win << b) | sym((u32)(m - 1 + r))) & wmask;
                if (i0 + r < e1) {
                    const u32 tp = win >> down;
                    atomicAdd(&hist[tp & (MSD_BINS - 1u)], 1u);
                    if (a.lsd) atomicAdd(&histb[tp >> MSD_D], 1u);
                }
            }
        }
    } else {
        for (u32 base = e0; base < e1; base += MSD_TILE) {
            const u32 valid = min(MSD_TILE, e1 - base);
            u64 elem[MSD_IPT];
            u32 dig[MSD_IPT];
            msd_load_tile<FROM_TEXT>(a, base, valid, elem, dig, shift2);
#pragma unroll
            for (int k = 0; k < MSD_IPT; ++k)
                if (msd_valid<FROM_TEXT>(base, valid, k, a.n)) atomicAdd(&hist[dig[k]], 1u);
        }
    }
    __syncthreads();
    // G1: digit-major (one row per digit: its offsets kernel scans rows); G2: range-major (one row per range)
    for (u32 i = tid; i < MSD_BINS; i += MSD_BLOCK) {
        if (FROM_TEXT) {
            a.T[(size_t)i * a.num_ranges1 + r] = hist[i];
            if (a.lsd) a.T2[(size_t)i * a.num_ranges1 + r] = histb[i];
        } else {
            a.T[(size_t)r * MSD_BINS + i] = hist[i];
        }
    }
}

// The first histogram pass when the codes do not exist yet (MsdFront): the same windows, read from the raw text through
// the byte -> code table (in LDS), and the codes of the thread's own 16 bytes written out on the way -- the recode pass
// and the alphabet pass before it (0.4 ms and a host round trip at n = 2^29) fold into this one.  A byte without a code
// raises *bad; the caller then throws the sort away.
__global__ __launch_bounds__(MSD_BLOCK) void msd_hist_raw_kernel(MsdArgs a)
{
    __shared__ u32 hist[MSD_BINS];
    __shared__ u32 histb[MSD_BINS];      // LSD order: the first digit (see msd_hist_kernel)
    __shared__ u8 s_lut[256];
    const u32 tid = threadIdx.x, r = blockIdx.x;
    if (r >= a.num_ranges1) return;
    const u32 e0 = r * a.tiles_per_range1 * MSD_TILE;
    const u64 end = (u64)(r + 1) * a.tiles_per_range1 * MSD_TILE;
    const u32 e1 = end < a.n ? (u32)end : a.n;
    for (u32 i = tid; i < MSD_BINS; i += MSD_BLOCK) hist[i] = histb[i] = 0;
    if (tid < 256) s_lut[tid] = a.lut[tid];
    __syncthreads();
    const int b = a.code_bits;
    const int top = a.lsd ? 2 * MSD_D : MSD_D;
    const int m = (top + b - 1) / b;
    const u32 wmask = (m * b >= 32) ? ~0u : ((1u << (m * b)) - 1u);
    const int down = m * b - top;
    auto tr = [&](u32 w) -> u32 {
        return (u32)s_lut[w & 0xffu] | ((u32)s_lut[(w >> 8) & 0xffu] << 8) | ((u32)s_lut[(w >> 16) & 0xffu] << 16) |
               ((u32)s_lut[w >> 24] << 24);
    };
    // 32 raw bytes at i: two 16-byte loads when they lie inside the text, byte by byte (zero past the end) at its end
    auto load32 = [&](u32 i, uint4 &lo, uint4 &hi) {
        if ((u64)i + 32 <= a.n) {
            const uint4 *p = reinterpret_cast<const uint4 *>(a.raw + i);
            lo = p[0];
            hi = p[1];
        } else {
            u32 w[8] = {};
            for (u32 k = 0; k < 32 && i + k < a.n; ++k) w[k >> 2] |= (u32)a.raw[i + k] << (8u * (k & 3u));
            lo = make_uint4(w[0], w[1], w[2], w[3]);
            hi = make_uint4(w[4], w[5], w[6], w[7]);
        }
    };
    bool bad = false;
    uint4 nlo = make_uint4(0, 0, 0, 0), nhi = nlo;
    if (e0 + tid * MSD_IPT < e1) load32(e0 + tid * MSD_IPT, nlo, nhi);
    for (u32 base = e0; base < e1; base += MSD_TILE) {
        const u32 i0 = base + tid * MSD_IPT;
        uint4 lo = nlo, hi = nhi;
        if ((u64)i0 + MSD_TILE < e1) load32(i0 + MSD_TILE, nlo, nhi);
        if (i0 >= e1) continue;
        lo = make_uint4(tr(lo.x), tr(lo.y), tr(lo.z), tr(lo.w));
        // of the sixteen bytes after my own the windows read the first m - 1: one word of them when that is <= 4 symbols
        // (every alphabet of >= 5 bits per symbol) -- the table lookups are what this pass spends its time on
        if (m <= 5) hi = make_uint4(tr(hi.x), 0u, 0u, 0u);
        else hi = make_uint4(tr(hi.x), tr(hi.y), tr(hi.z), tr(hi.w));
        // my own 16 bytes: codes out, and every one of them inside the text must have got a code
        const u32 own = min(16u, a.n - i0);
        if (own == 16) {
            *reinterpret_cast<uint4 *>(a.codes_out + i0) = lo;
            const u32 z = ((lo.x - 0x01010101u) & ~lo.x) | ((lo.y - 0x01010101u) & ~lo.y) | ((lo.z - 0x01010101u) & ~lo.z) |
                          ((lo.w - 0x01010101u) & ~lo.w);
            bad |= (z & 0x80808080u) != 0;
        } else {
            const u32 w[4] = {lo.x, lo.y, lo.z, lo.w};
            for (u32 k = 0; k < own; ++k) {
                const u8 c = (u8)(w[k >> 2] >> (8u * (k & 3u)));
                a.codes_out[i0 + k] = c;
                bad |= c == 0;
            }
            // (a raw byte past the end reads as 0 and translates to lut[0]: the window must see 0 there)
            u32 ww[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            for (u32 k = own; k < 32; ++k) ww[k >> 2] &= ~(0xffu << (8u * (k & 3u)));
            lo = make_uint4(ww[0], ww[1], ww[2], ww[3]);
            hi = make_uint4(ww[4], ww[5], ww[6], ww[7]);
        }
        if (own == 16 && (u64)i0 + 32 > a.n) {            // the window's second half crosses the end of the text
            u32 ww[4] = {hi.x, hi.y, hi.z, hi.w};
            for (u32 k = 0; k < 16; ++k)
                if (i0 + 16 + k >= a.n) ww[k >> 2] &= ~(0xffu << (8u * (k & 3u)));
            hi = make_uint4(ww[0], ww[1], ww[2], ww[3]);
        }
        const u64 q[4] = {(u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32),
                          (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32)};
        auto sym = [&](u32 j) -> u32 { return (u32)(q[j >> 3] >> ((j & 7u) * 8u)) & 0xffu; };
        u32 win = 0;
        for (int t = 0; t < m; ++t) win = (win << b) | sym((u32)t);
#pragma unroll
        for (int k = 0; k < MSD_IPT; ++k) {
            if (k > 0) win = ((win << b) | sym((u32)(m - 1 + k))) & wmask;
            if (i0 + k < e1) {
                const u32 tp = win >> down;
                atomicAdd(&hist[tp & (MSD_BINS - 1u)], 1u);
                if (a.lsd) atomicAdd(&histb[tp >> MSD_D], 1u);
            }
        }
    }
    if (__ballot(bad) && (tid & 63u) == 0) atomicOr(a.bad, 1u);
    __syncthreads();
    for (u32 i = tid; i < MSD_BINS; i += MSD_BLOCK) {
        a.T[(size_t)i * a.num_ranges1 + r] = hist[i];
        if (a.lsd) a.T2[(size_t)i * a.num_ranges1 + r] = histb[i];
    }
}

// G1 offsets, step 1: one workgroup per digit turns its row of per-range counts into exclusive prefixes
// and leaves the digit's total; step 2 (one workgroup) scans the totals into the bucket starts J1.
__global__ __launch_bounds__(256) void msd_offsets1_kernel(u32 *T, u32 num_ranges, u32 *totals)
{
    __shared__ u32 scr[256 / kWave + 1];
    const u32 d = blockIdx.x, tid = threadIdx.x;
    u32 *row = T + (size_t)d * num_ranges;
    u32 v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 r = tid * 4 + j;
        v[j] = r < num_ranges ? row[r] : 0u;
        sum += v[j];
    }
    u32 total = 0;
    u32 run = block_excl_sum<256 / kWave>(sum, scr, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u32 r = tid * 4 + j;
        if (r < num_ranges) row[r] = run;
        run += v[j];
    }
    if (tid == 0) totals[d] = total;
}
__global__ __launch_bounds__(MSD_BINS) void msd_offsets1b_kernel(const u32 *totals, u32 *J1, u32 n)
{
    __shared__ u32 scr[MSD_BINS / kWave + 1];
    const u32 d = threadIdx.x;
    J1[d] = block_excl_sum<MSD_BINS / kWave>(totals[d], scr, nullptr);
    if (d == 0) J1[MSD_BINS] = n;
}

// One workgroup per segment (G1: the whole input; G2: one G1 bucket), thread = digit:
// T[r][d] := global offset of (range r, digit d); joint[seg * 1024 + d] := start of bucket (seg, d).
__global__ __launch_bounds__(MSD_BINS) void msd_offsets_kernel(u32 *T, const u32 *seg_first, const u32 *seg_start, u32 *joint,
                                                                u32 num_ranges_fixed, u32 n, u32 nseg)
{
    __shared__ u32 scr[MSD_BINS / kWave + 1];
    const u32 seg = blockIdx.x, d = threadIdx.x;
    const u32 r0 = seg_first ? seg_first[seg] : 0u;
    const u32 r1 = seg_first ? seg_first[seg + 1] : num_ranges_fixed;
    const u32 base = seg_start ? seg_start[seg] : 0u;
    u32 run = 0;
    for (u32 r = r0; r < r1; ++r) {
        const u32 c = T[(size_t)r * MSD_BINS + d];
        T[(size_t)r * MSD_BINS + d] = run;
        run += c;
    }
    const u32 binbase = base + block_excl_sum<MSD_BINS / kWave>(run, scr, nullptr);
    joint[(size_t)seg * MSD_BINS + d] = binbase;
    if (seg == nseg - 1 && d == 0) joint[(size_t)nseg * MSD_BINS] = n;
    for (u32 r = r0; r < r1; ++r) T[(size_t)r * MSD_BINS + d] += binbase;
}

// G2 ranges: pieces of <= MSD_G2_RANGE elements of one G1 bucket.  One workgroup, thread = bucket.
__global__ __launch_bounds__(MSD_BINS) void msd_ranges_kernel(const u32 *J1, MsdRange *ranges, u32 *seg_first, u32 *counters)
{
    __shared__ u32 scr[MSD_BINS / kWave + 1];
    const u32 seg = threadIdx.x;
    const u32 s = J1[seg], e = J1[seg + 1];
    const u32 nr = (e - s + MSD_G2_RANGE - 1) / MSD_G2_RANGE;
    u32 total = 0;
    const u32 first = block_excl_sum<MSD_BINS / kWave>(nr, scr, &total);
    seg_first[seg] = first;
    if (seg == MSD_BINS - 1) seg_first[MSD_BINS] = total;
    if (seg == 0) counters[0] = total;
    for (u32 k = 0; k < nr; ++k) {
        const u32 rs = s + k * MSD_G2_RANGE;
        ranges[first + k] = MsdRange{seg, rs, min(e, rs + MSD_G2_RANGE)};
    }
}

template <bool FROM_TEXT>
__global__ __launch_bounds__(MSD_BLOCK, 4) void msd_scatter_kernel(MsdArgs a)
{
    // (79.9 KB of LDS: both instantiations fit twice into a CU)
    __shared__ __attribute__((aligned(16))) u64 exch[MSD_TILE];
    __shared__ u32 hist[MSD_BINS], s_delta[MSD_BINS], s_off[MSD_BINS];
    __shared__ u16 s_start[MSD_BINS];                 // 16-bit (a tile has 8192 slots): the G2 kernel then fits twice into a CU's LDS
    __shared__ u32 scr[MSD_WAVES + 1];
    const u32 tid = threadIdx.x, r = blockIdx.x;
    u32 e0, e1;
    u32 tag0 = 0, tag1 = 0;      // G2: what the elements of bins 2 tid, 2 tid + 1 are tagged with
    if (FROM_TEXT) {
        if (r >= a.num_ranges1) return;
        e0 = r * a.tiles_per_range1 * MSD_TILE;
        const u64 end = (u64)(r + 1) * a.tiles_per_range1 * MSD_TILE;
        e1 = end < a.n ? (u32)end : a.n;
    } else {
        if (r >= a.counters[0]) return;
        e0 = a.ranges2[r].start;
        e1 = a.ranges2[r].end;
        // The element leaves G2 as [ tag | remaining key bits | index ], tag = low 11 bits of its joint bucket's number
        // among the non-empty buckets (known before this pass: the plan runs on G2's histogram): the local sort
        // reads the bucket of an element from the element (msd_local_*: no table of bucket starts, no search).
        // The tag of a bin rides in the high half of its counter word -- the returning atomic of the ranking brings it
        // along for nothing, the output loop reads it with the bin's offset.
        const u64 *dn = a.dense + (size_t)a.ranges2[r].seg * MSD_BINS;
        tag0 = ((u32)dn[2 * tid] & (MSD_TAG_SPAN - 1u)) << 16;
        tag1 = ((u32)dn[2 * tid + 1] & (MSD_TAG_SPAN - 1u)) << 16;
        hist[2 * tid] = tag0;
        hist[2 * tid + 1] = tag1;
    }
    for (u32 i = tid; i < MSD_BINS; i += MSD_BLOCK) {
        if (FROM_TEXT) hist[i] = 0;
        s_off[i] = FROM_TEXT ? a.T[(size_t)i * a.num_ranges1 + r] + a.J1[i] : a.T[(size_t)r * MSD_BINS + i];
    }
    __syncthreads();
    const int shift2 = a.idx_bits + a.key_bits - 2 * MSD_D;
    const u64 low_mask2 = (1ull << shift2) - 1ull;
    for (u32 base = e0; base < e1; base += MSD_TILE) {
        const u32 valid = min(MSD_TILE, e1 - base);
        u64 elem[MSD_IPT];
        u32 dig[MSD_IPT];
        u32 rank[MSD_IPT];
        msd_load_tile<FROM_TEXT>(a, base, valid, elem, dig, shift2);
#pragma unroll
        for (int k = 0; k < MSD_IPT; ++k)
            rank[k] = msd_valid<FROM_TEXT>(base, valid, k, a.n) ? (atomicAdd(&hist[dig[k]], 1u) & 0xffffu) : 0u;
        __syncthreads();                                    // (A) counts complete; previous tile fully written out
        {
            // exclusive scan over the 1024 bins, two adjacent bins per thread
            const u32 c0 = hist[2 * tid] & 0xffffu, c1 = hist[2 * tid + 1] & 0xffffu;
            const u32 ex = block_excl_sum<MSD_WAVES>(c0 + c1, scr, nullptr);
            s_start[2 * tid] = (u16)ex;
            s_start[2 * tid + 1] = (u16)(ex + c0);
            const u32 o0 = s_off[2 * tid], o1 = s_off[2 * tid + 1];
            s_delta[2 * tid] = o0 - ex;
            s_delta[2 * tid + 1] = o1 - (ex + c0);
            s_off[2 * tid] = o0 + c0;
            s_off[2 * tid + 1] = o1 + c1;
            hist[2 * tid] = tag0;
            hist[2 * tid + 1] = tag1;
        }
        __syncthreads();                                    // (B) bin starts published
#pragma unroll
        for (int k = 0; k < MSD_IPT; ++k) {
            if (msd_valid<FROM_TEXT>(base, valid, k, a.n)) {
                const u32 lp = (u32)s_start[dig[k]] + rank[k];
                // G1's element no longer holds its digit, and the output loop needs it: through LDS it travels as
                // [key rest | digit | position in the tile] (13 bits instead of the suffix index, which is base + position)
                if (FROM_TEXT) exch[lp] = ((elem[k] >> a.idx_bits) << 23) | ((u64)dig[k] << 13) | (u64)(tid * MSD_IPT + k);
                else exch[lp] = elem[k];
            }
        }
        __syncthreads();                                    // (C) tile in bin order
#pragma unroll
        for (int k = 0; k < MSD_IPT; ++k) {
            const u32 p = k * MSD_BLOCK + tid;
            if (p < valid) {
                u64 e = exch[p];
                u32 d;
                if (FROM_TEXT) {
                    d = (u32)(e >> 13) & (MSD_BINS - 1u);
                    e = ((e >> 23) << a.idx_bits) | (u64)(base + ((u32)e & (MSD_TILE - 1u)));
                } else {
                    d = (u32)(e >> shift2) & (MSD_BINS - 1u);
                    e = (e & low_mask2) | ((u64)(hist[d] >> 16) << shift2);
                }
                a.out[s_delta[d] + p] = e;
            }
        }
    }
}

// The same pass over tiles of 16384 elements (1024 threads x 16): twice as many elements per bin and tile, so the runs
// the output loop writes are 16 x 8 = 128 bytes on average -- whole lines instead of half lines; the pass is bound by
// the 128-byte lines it touches (docs/history 4.3).  LDS stages 8192 elements at a time: the tile goes through in two
// pieces by destination position.  (The whole tile in one piece -- 128 KiB of the CU's 160, one round of writes, two
// barriers fewer -- was measured in both kernels and is no faster: DESIGN 4.2.)
constexpr int MSD_PIECES2 = MSD_TILE2 / MSD_TILE;    // 2

template <bool FROM_TEXT, int BLOCK, bool LSD = false>
__global__ __launch_bounds__(BLOCK) void msd_scatter2_kernel(MsdArgs a)
{
    constexpr int IPT = MSD_TILE2 / BLOCK;               // 16 (1024 threads) or 32 (512)
    constexpr int BPT = MSD_BINS / BLOCK;                // bins per thread in the scan
    __shared__ __attribute__((aligned(16))) u64 exch[MSD_TILE];
    __shared__ u32 hist[MSD_BINS], s_delta[MSD_BINS], s_off[MSD_BINS];
    __shared__ u16 s_start[MSD_BINS];
    __shared__ u32 scr[BLOCK / kWave + 1];
    const u32 tid = threadIdx.x, r = blockIdx.x;
    u32 e0, e1;
    u32 tag[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) tag[j] = 0;
    if (FROM_TEXT) {
        if (r >= a.num_ranges1) return;
        e0 = r * a.tiles_per_range1 * MSD_TILE;
        const u64 end = (u64)(r + 1) * a.tiles_per_range1 * MSD_TILE;
        e1 = end < a.n ? (u32)end : a.n;
    } else {
        if (r >= a.counters[0]) return;
        e0 = a.ranges2[r].start;
        e1 = a.ranges2[r].end;
#pragma unroll
        for (int j = 0; j < BPT; ++j)      // see msd_scatter_kernel
            tag[j] = ((u32)a.dense[(size_t)a.ranges2[r].seg * MSD_BINS + BPT * tid + j] & (MSD_TAG_SPAN - 1u)) << 16;
    }
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const u32 i = BPT * tid + j;
        hist[i] = tag[j];
        s_off[i] = FROM_TEXT ? a.T[(size_t)i * a.num_ranges1 + r] + a.J1[i] : a.T[(size_t)r * MSD_BINS + i];
    }
    __syncthreads();
    const int shift2 = a.idx_bits + a.key_bits - 2 * MSD_D;
    const u64 low_mask2 = (1ull << shift2) - 1ull;
    const int rest_bits = a.key_bits - MSD_D;
    const u64 rest_mask = (1ull << rest_bits) - 1ull;
    // From the text, the code words are loaded one tile ahead: all sixteen waves of the CU's only workgroup are in the
    // same phase, so a load issued where it is used is a trip to memory nobody hides.  The words of the next tile are
    // asked for once the registers of the current one are free (behind the staging writes of its second piece) and land
    // under that piece's output and the next tile's first instructions.
    uint4 ahead[FROM_TEXT ? IPT / 16 : 1][2] = {};
    auto load_ahead = [&](u32 b) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < IPT / 16; ++g) {
            const u32 i0 = b + tid * IPT + g * 16;
            if (i0 < a.n) text_keys16_load(a.codes, i0, ahead[g][0], ahead[g][1]);
        }
    };
    if (FROM_TEXT) load_ahead(e0);
    for (u32 base = e0; base < e1; base += MSD_TILE2) {
        const u32 valid = min(MSD_TILE2, e1 - base);
        u64 elem[IPT];
        u32 lp[IPT];          // position in the tile (before the scan: rank inside the bin), digit in the top 10 bits
        if (FROM_TEXT) {
#pragma unroll
            for (int g = 0; g < IPT / 16; ++g) {
                keep_load(ahead[g][0]);      // (or the compiler sinks the loads to this place, their use)
                keep_load(ahead[g][1]);
            }
            // (the thread's first position, opaque per tile: hoisted out of the loop, "first position | k" is sixteen
            //  registers held across every phase, and the kernel spills)
            u32 pos0 = tid * IPT;
            asm volatile("" : "+v"(pos0));
#pragma unroll
            for (int g = 0; g < IPT / 16; ++g) {
                const u32 i0 = base + pos0 + g * 16;
                u64 key[16] = {};
                if (i0 < a.n)
                    text_keys16_pack(ahead[g][0], ahead[g][1], i0, a.code_bits, a.key_chars, a.plus_one, a.key_drop, a.n, key);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const u32 pos = pos0 + g * 16 + k;
                    u32 d;
                    u64 keep;                                   // the K - 10 key bits the element carries on
                    if (LSD) {                                  // the pass's digit is the SECOND ten bits; the first ten stay
                        d = (u32)(key[k] >> (rest_bits - MSD_D)) & (MSD_BINS - 1u);
                        keep = ((key[k] >> rest_bits) << (rest_bits - MSD_D)) | (key[k] & (rest_mask >> MSD_D));
                    } else {
                        d = (u32)(key[k] >> rest_bits) & (MSD_BINS - 1u);
                        keep = key[k] & rest_mask;
                    }
                    // through LDS: [key rest | digit | position in the tile]; the suffix index is base + position
                    elem[g * 16 + k] = (keep << 24) | ((u64)d << 14) | (u64)pos;
                    lp[g * 16 + k] = pos < valid ? ((atomicAdd(&hist[d], 1u) & 0xffffu) | (d << 22)) : 0xffffffffu;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const u32 p = k * BLOCK + tid;
                elem[k] = p < valid ? a.in[base + p] : 0ull;
            }
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const u32 p = k * BLOCK + tid;
                const u32 d = (u32)(elem[k] >> shift2) & (MSD_BINS - 1u);
                lp[k] = p < valid ? ((atomicAdd(&hist[d], 1u) & 0xffffu) | (d << 22)) : 0xffffffffu;
            }
        }
        __syncthreads();                                    // (A) counts complete; previous tile fully written out
        {
            u32 c[BPT], sum = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                c[j] = hist[BPT * tid + j] & 0xffffu;
                sum += c[j];
            }
            u32 ex = block_excl_sum_lean<BLOCK / kWave>(sum, scr);
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const u32 i = BPT * tid + j;
                s_start[i] = (u16)ex;
                const u32 o = s_off[i];
                s_delta[i] = o - ex;
                s_off[i] = o + c[j];
                hist[i] = tag[j];
                ex += c[j];
            }
        }
        __syncthreads();                                    // (B) bin starts published
#pragma unroll
        for (int k = 0; k < IPT; ++k)
            if (lp[k] != 0xffffffffu) lp[k] = (lp[k] & 0xffffu) + (u32)s_start[lp[k] >> 22];
#pragma unroll
        for (int h = 0; h < MSD_PIECES2; ++h) {
            if (h * MSD_TILE >= valid) break;
            if (h) __syncthreads();                         // the piece before this one is written out
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const u32 q = lp[k] - h * MSD_TILE;
                if (q < MSD_TILE) exch[q] = elem[k];
            }
            // (a tile with a successor in its range is full: its last piece is the last one of the loop.  elem and lp are
            //  dead from here: room for the words)
            if (FROM_TEXT && h == MSD_PIECES2 - 1 && (u64)base + MSD_TILE2 < e1) load_ahead(base + MSD_TILE2);
            lds_barrier();                                  // (C) the piece in bin order; the loads stay in flight
#pragma unroll
            for (int k = 0; k < (int)(MSD_TILE / BLOCK); ++k) {
                const u32 q = k * BLOCK + tid, p = h * MSD_TILE + q;
                if (p < valid) {
                    u64 e = exch[q];
                    u32 d;
                    if (FROM_TEXT) {
                        d = (u32)(e >> 14) & (MSD_BINS - 1u);
                        e = ((e >> 24) << a.idx_bits) | (u64)(base + ((u32)e & (MSD_TILE2 - 1u)));
                    } else {
                        d = (u32)(e >> shift2) & (MSD_BINS - 1u);
                        e = (e & low_mask2) | ((u64)(hist[d] >> 16) << shift2);
                    }
                    a.out[s_delta[d] + p] = e;
                }
            }
        }
    }
}

// ---- decoupled look-back: where does (tile, bin) go? -------------------------------------------------------
// A look-back word: two state bits over a 30-bit number (n < 2^30 on this path).  A: the tile's own count of the bin;
// P: where the bin stands after the tile -- start of the bin's bucket + everything up to and including the tile.
// One 4-byte word per (tile, bin) carries state and number, so nothing needs ordering beyond the word itself: relaxed
// device-scope accesses.  Tiles are handed out by an atomic ticket: every predecessor of a waiting tile is running.
constexpr u32 LB_A = 1u << 30, LB_P = 2u << 30, LB_STATE = 3u << 30, LB_VALUE = LB_A - 1u;
constexpr int LB_WINDOW = 4;                         // predecessors asked per trip (their loads are in flight together)

// thread = bin.  lb_begin publishes the tile's count c and asks the first window of predecessors; lb_finish adds up what
// they published, back to the nearest running total (asking again while it must), publishes the tile's own running total
// and returns where the tile's elements of the bin start.  first: the bin's bucket start (tile 0).  Between the two the
// caller does what does not depend on the answer (scanning its bins, staging its first piece into LDS): the round trip of
// the first window costs nothing then (tests/tools/lookback_micro.hip: 2.34 -> 2.26 ms for the pass).
struct LbAsk {
    u32 v[LB_WINDOW];
};
__device__ __forceinline__ void lb_ask(const u32 *status, u32 p, LbAsk &q)
{
#pragma unroll
    for (u32 w = 0; w < (u32)LB_WINDOW; ++w) {
        const u32 r = p > w ? p - 1 - w : 0u;
        q.v[w] = __hip_atomic_load(&status[(size_t)r * MSD_BINS + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void lb_begin(u32 *status, u32 t, u32 c, LbAsk &q)
{
    if (t == 0) return;
    __hip_atomic_store(&status[(size_t)t * MSD_BINS + threadIdx.x], LB_A | c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lb_ask(status, t, q);
}
__device__ __forceinline__ u32 lb_finish(u32 *status, u32 t, u32 c, u32 first, LbAsk &q)
{
    u32 off = first;
    if (t != 0) {
        u32 sum = 0, p = t;                           // predecessors not yet added: the next one is p - 1
        for (;;) {
            const u32 p0 = p;
            bool stop = false, done = false;
#pragma unroll
            for (u32 w = 0; w < (u32)LB_WINDOW; ++w) {
                if (!stop && w < p0) {
                    const u32 st = q.v[w] & LB_STATE;
                    if (st == 0) {
                        stop = true;                  // not published yet: ask again from here
                    } else {
                        sum += q.v[w] & LB_VALUE;
                        --p;
                        if (st == LB_P) done = stop = true;
                    }
                }
            }
            if (done || p == 0) break;                // (tile 0 publishes P: p == 0 is never the way out)
            lb_ask(status, p, q);
        }
        off = sum;
    }
    __hip_atomic_store(&status[(size_t)t * MSD_BINS + threadIdx.x], LB_P | (off + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return off;
}

// ---- second pass in one sweep: decoupled look-back (LSD order) ---------------------------------------

// Tiles of the look-back pass: every d-region cut into pieces of MSD_TILE2 elements.  The regions are RENUMBERED on the way:
// the non-empty ones first, 0 .. D - 1 in digit order, then the empty ones (each still gets one tile of nothing: it owes
// its row of the joint table).  From here on "d" is that number: a digit value that never occurs in the text (a quarter
// of the 1024 for a 39-symbol alphabet in 6-bit codes) leaves no hole in the numbering of the joint buckets (b, d), which
// is what lets the local sort take "tag - tag of the tile's first bucket" as the bucket's number inside its tile.
// One workgroup, thread = region.
__global__ __launch_bounds__(MSD_BINS) void msd_tiles2_kernel(const u32 *J1, MsdTile2 *tiles, u32 *counters)
{
    __shared__ u32 scr[MSD_BINS / kWave + 1];
    const u32 d = threadIdx.x;
    const u32 s = J1[d], e = J1[d + 1];
    const u32 nr = (e - s + MSD_TILE2 - 1) / MSD_TILE2;
    u32 total = 0, D = 0;
    const u32 first = block_excl_sum<MSD_BINS / kWave>(nr, scr, &total);
    const u32 dn = block_excl_sum<MSD_BINS / kWave>(nr ? 1u : 0u, scr, &D);      // non-empty regions below this one
    if (d == 0) counters[0] = total + (MSD_BINS - D);
    if (nr == 0) {
        const u32 dd = D + (d - dn);                                               // (d - dn: empty regions below)
        tiles[total + (d - dn)] = MsdTile2{s, 0u, dd | 0x80000000u};
    }
    for (u32 k = 0; k < nr; ++k) {
        const u32 ts = s + k * MSD_TILE2;
        tiles[first + k] = MsdTile2{ts, min(MSD_TILE2, e - ts), dn | (k + 1 == nr ? 0x80000000u : 0u)};
    }
}

// Persistent workgroups, tiles by ticket (a waiting tile's predecessors all hold earlier tickets, hence run).  Per tile:
// load, rank with one returning LDS atomic per element, publish the 1024 counts, add up the predecessors' (thread =
// bin; one 4-byte word per (tile, bin) carries state and number, so nothing needs ordering beyond the word itself:
// relaxed device-scope accesses), publish the running totals, stage through LDS in two pieces, write.  Measured in
// tests/tools/lookback_micro.hip at n = 2^29: 2.5 ms against 0.88 + 2.2 ms for histogram pass + scatter from a table;
// a tile asks 5 trips of 4 rows on average (one chain over all tiles; 4 .. 64 chains side by side read fewer rows and
// were no faster: neighbouring tiles then write to far-apart places).
__global__ __launch_bounds__(1024) void msd_scatter_lb_kernel(MsdArgs a)
{
    constexpr int BLOCK = 1024;
    constexpr int IPT = MSD_TILE2 / BLOCK;               // 16
    __shared__ __attribute__((aligned(16))) u64 exch[MSD_TILE];
    __shared__ u32 hist[MSD_BINS], s_delta[MSD_BINS];
    __shared__ u16 s_start[MSD_BINS];
    __shared__ u32 scr[BLOCK / kWave + 1];
    __shared__ u32 s_ticket;
    const u32 tid = threadIdx.x;
    const u32 nt = a.counters[0];
    const int shift2 = a.idx_bits + a.key_bits - 2 * MSD_D;      // the first digit sits right above [remaining key bits | index]
    const u64 low_mask2 = (1ull << shift2) - 1ull;
    hist[tid] = 0;
    __syncthreads();
    for (;;) {
        if (tid == 0) s_ticket = atomicAdd(&a.counters[8], 1u);
        __syncthreads();
        const u32 t = s_ticket;
        if (t >= nt) break;
        const MsdTile2 td = a.tiles2[t];
        const u32 base = td.start, valid = td.count;
        u64 elem[IPT];
        u32 lp[IPT];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const u32 p = k * BLOCK + tid;
            elem[k] = p < valid ? a.in[base + p] : 0ull;
        }
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const u32 p = k * BLOCK + tid;
            const u32 d = (u32)(elem[k] >> shift2) & (MSD_BINS - 1u);
            lp[k] = p < valid ? (atomicAdd(&hist[d], 1u) | (d << 22)) : 0xffffffffu;
        }
        __syncthreads();                                    // (A) counts complete; previous tile fully written out
        const u32 c = hist[tid];
        LbAsk ask;
        lb_begin(a.status, t, c, ask);                      // my counts are out, the first window of predecessors is on its way
        const u32 ex = block_excl_sum<BLOCK / kWave>(c, scr, nullptr);
        s_start[tid] = (u16)ex;
        hist[tid] = 0;
        __syncthreads();                                    // (B) bin starts published
        // what the element leaves as: [ tag | remaining key bits | index ], tag = joint bucket number mod 64 = d mod 64
        const u64 tag = (u64)(td.d_last & (MSD_RAW_TAG_SPAN - 1u)) << shift2;
#pragma unroll
        for (int k = 0; k < IPT; ++k)
            if (lp[k] != 0xffffffffu) lp[k] = (lp[k] & 0xffffu) + (u32)s_start[lp[k] >> 22];
#pragma unroll
        for (int h = 0; h < MSD_PIECES2; ++h) {
            if (h && h * MSD_TILE >= valid) break;
            if (h) __syncthreads();                         // the piece before this one is written out
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const u32 q = lp[k] - h * MSD_TILE;
                if (q < MSD_TILE) exch[q] = elem[k];
            }
            if (h == 0) {
                // only the OUTPUT needs to know where the bins go: the look-back is settled behind the staging
                if (t == 0 && tid == 0) a.J[0] = 0;
                const u32 off = lb_finish(a.status, t, c, a.Jb[tid], ask);
                // the last tile of d-region d: where bin b stands now is the end of joint bucket (b, d)
                if (td.d_last >> 31) a.J[(size_t)tid * MSD_BINS + (td.d_last & (MSD_BINS - 1u)) + 1u] = off + c;
                s_delta[tid] = off - ex;
            }
            __syncthreads();                                // (C) the piece in bin order
#pragma unroll
            for (int k = 0; k < (int)(MSD_TILE / BLOCK); ++k) {
                const u32 q = k * BLOCK + tid, p = h * MSD_TILE + q;
                if (p < valid) {
                    const u64 e = exch[q];
                    const u32 d = (u32)(e >> shift2) & (MSD_BINS - 1u);
                    a.out[s_delta[d] + p] = (e & low_mask2) | tag;
                }
            }
        }
    }
}

// ---- tile plan ---------------------------------------------------------------------------------

struct InNonEmpty {
    const u32 *J;
    __device__ u64 operator()(u64 j) const { return J[j + 1] > J[j] ? 1u : 0u; }
};

// compact the starts of the non-empty joint buckets; largest bucket
// (cj, LSD order: the joint bucket number of every non-empty bucket -- the tile rule and the tiles' tags need it)
__global__ __launch_bounds__(256) void msd_compact_kernel(const u32 *J, u32 nb, const u64 *rank, u32 *cstart, u32 *counters, u32 *cj)
{
    u32 mx = 0;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += gridDim.x * blockDim.x) {
        const u32 s = J[j], e = J[j + 1];
        if (e > s) {
            cstart[rank[j]] = s;
            if (cj) cj[rank[j]] = j;
            mx = max(mx, e - s);
        }
    }
    mx = wave_incl_max(mx);
    if (lane_id() == kWave - 1 && mx) atomicMax(&counters[1], mx);
}

// Tiles: the (non-empty) buckets that start inside one MSD_WIN window form a tile (< MSD_WIN + MSD_MAX_BUCKET
// elements); when that exceeds MSD_TILE_CAP the window's last bucket becomes a tile of its own (what is left
// ends before the window does: < MSD_WIN).  A tile stays inside one aligned block of MSD_TAG_SPAN buckets.  Every decision looks at
// one window only, so all of them are taken in parallel -- and tiles come out at ~5 500 elements on `lines`
// instead of the 4 096 of a plain "one tile per 4096-slot window" rule (a fifth fewer tiles).
struct TilePlan {
    u32 win, cap;      // window of the rule above; elements a tile holds at most
    const u32 *cj;     // LSD order: joint bucket numbers of the non-empty buckets -- a tile stays inside one aligned block of
                       // MSD_RAW_TAG_SPAN joint buckets (else: of MSD_TAG_SPAN non-empty ones)
};
__device__ __forceinline__ bool msd_tile_head(const u32 *cstart, u32 ne, u32 n, u32 k, TilePlan tp)
{
    if (tp.cj) {
        if (k == 0 || (tp.cj[k] >> MSD_RAW_TAG_BITS) != (tp.cj[k - 1] >> MSD_RAW_TAG_BITS)) return true;
    } else if ((k & (MSD_TAG_SPAN - 1u)) == 0) {
        return true;
    }
    const u32 w = cstart[k] / tp.win;
    if (cstart[k - 1] / tp.win != w) return true;                        // first bucket of its window
    if (k + 1 < ne && cstart[k + 1] / tp.win == w) return false;         // neither first nor last
    u32 lo = 0, hi = k;                                                  // first bucket of the window: start >= w * WIN
    const u32 ws = w * tp.win;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (cstart[mid] < ws) lo = mid + 1; else hi = mid;
    }
    const u32 end = k + 1 < ne ? cstart[k + 1] : n;
    return end - cstart[lo] > tp.cap;                                    // the window does not fit: its last bucket goes alone
}

struct InTileHead {
    const u32 *cstart;
    u32 ne, n;
    TilePlan tp;
    __device__ u64 operator()(u64 k) const { return msd_tile_head(cstart, ne, n, (u32)k, tp) ? 1u : 0u; }
};

// The same with the number of non-empty buckets read on the device (LSD order: the whole plan is launched without a
// host round trip; the scan runs over all 2^20 bucket numbers, those from *nep on count nothing).
struct InTileHeadDev {
    const u32 *cstart;
    const u64 *nep;
    u32 n;
    TilePlan tp;
    __device__ u64 operator()(u64 k) const
    {
        const u32 ne = (u32)*nep;
        return (k < ne && msd_tile_head(cstart, ne, n, (u32)k, tp)) ? 1u : 0u;
    }
};
__global__ __launch_bounds__(256) void msd_tiles_dev_kernel(const u32 *cstart, const u64 *nep, u32 n, const u64 *rank, const u64 *total,
                                                              u32 *tile_first, TilePlan tp)
{
    const u32 ne = (u32)*nep;
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_first[*total] = ne;      // sentinel behind the last tile
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < ne; k += gridDim.x * blockDim.x) {
        if (msd_tile_head(cstart, ne, n, k, tp)) tile_first[rank[k]] = k;
    }
}

__global__ __launch_bounds__(256) void msd_tiles_kernel(const u32 *cstart, u32 ne, u32 n, const u64 *rank, const u64 *total,
                                                          u32 *tile_first, TilePlan tp)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_first[*total] = ne;      // sentinel behind the last tile
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < ne; k += gridDim.x * blockDim.x) {
        if (msd_tile_head(cstart, ne, n, k, tp)) tile_first[rank[k]] = k;
    }
}

// ---- output of a sorted tile ------------------------------------------------------------------------

// Where the still-tied suffixes go when the caller wants the active list of the first rerank straight
// from the local sort (instead of re-reading 4 n bytes of flagged suffix array twice).  Ties are rare on
// the texts this path takes (a handful per tile), so the sorting workgroup only drops a record per tied
// element -- SA slot and suffix, bit 31 of the suffix word = "tied with my predecessor" -- into the
// tile's block of the staging arrays, in whatever order the lanes get there (one LDS atomic each; the
// block starts at the tile's own first SA slot: no allocation, no overlap).  msd_gather_kernel then
// orders every block by slot with a bitmap, derives the group heads and packs the blocks in tile order.
struct MsdEmit {
    u32 *st_pos, *st_idx;            // staging (capacity n each)
    u32 *blk_cnt;                    // [tiles] records of every tile
};

// exch[0 .. count) is the sorted tile (position p <-> thread p % 512, row p / 512).  Writes the suffix
// indices to sa_out[e0 ..]; without `em` bit 31 marks "same key as my predecessor" (the contract of
// suffix_sort_flags), with it the array is written clean and a record goes out for every element that
// is tied with a neighbour (it or its successor carries the flag; a tile starts at a bucket boundary,
// so groups never cross tiles).  s_count: one zeroed word of LDS; the caller's next barrier publishes it.
__device__ __forceinline__ void msd_emit_tile(const u64 *exch, u32 count, u32 e0, int idx_bits, u32 *sa_out, const MsdEmit *em,
                                              u32 *s_count)
{
    const u32 tid = threadIdx.x, lane = tid & 63u;
    const u32 imask = (u32)((1ull << idx_bits) - 1ull);
    const u32 rows = (count + MSD_BLOCK - 1) / MSD_BLOCK;
#pragma unroll 1
    for (u32 r = 0; r < rows; ++r) {
        const u32 p = r * MSD_BLOCK + tid;
        const bool valid = p < count;
        u64 x = 0;
        bool tie = false;
        if (valid) {
            x = exch[p];
            tie = p > 0 && (exch[p - 1] >> idx_bits) == (x >> idx_bits);
            sa_out[e0 + p] = ((u32)x & imask) | ((tie && em == nullptr) ? 0x80000000u : 0u);
        }
        if (em != nullptr) {
            const u64 tm = __ballot(tie);
            // my successor's flag: the next lane's, or (lane 63) one more look into LDS
            const bool tie_next = lane < 63 ? ((tm >> (lane + 1)) & 1ull) != 0
                                            : (p + 1 < count && (exch[p + 1] >> idx_bits) == (x >> idx_bits));
            if (valid && (tie || tie_next)) {
                const u32 slot = e0 + atomicAdd(s_count, 1u);
                em->st_pos[slot] = e0 + p;
                em->st_idx[slot] = ((u32)x & imask) | (tie ? 0x80000000u : 0u);
            }
        }
    }
}

// blk_cnt[t] = records of tile t in its low half (a tile has < 8192), in the high half the records msd_finish_kernel has
// dropped.  The scan adds both up at once -- records in the low word of its 64-bit sums, finished suffixes in the high word
// (one counter for all tiles would be a hundred thousand atomics on one address: 1.1 ms at n = 2^29, measured).
struct InBlkCnt {
    const u32 *c;
    __device__ u64 operator()(u64 t) const { return (u64)(c[t] & 0xffffu) | ((u64)(c[t] >> 16) << 32); }
};

// One wavefront per tile: the tile's records (unordered) -> the active list of the first rerank in slot
// order: (SA slot, suffix, 1 + SA slot of the group's head).  A bitmap of the tile's occupied slots ranks
// a record by the bits below its slot; a second bitmap of the untied ones (group heads -- the head of a
// tied element is itself active, so it has a record) gives its head as the nearest set bit at or below.
// O(records) whatever the tile looks like.
constexpr u32 GA_WORDS = MSD_TILE / 32;      // 256 words per bitmap
__global__ __launch_bounds__(256) void msd_gather_kernel(const MsdTile *tiles, const u32 *blk_cnt, const u64 *dst_off, u32 nt,
                                                           const u32 *st_pos, const u32 *st_idx, u32 *pos, u32 *idx, u32 *grp)
{
    __shared__ u32 s_occ[4][GA_WORDS], s_head[4][GA_WORDS], s_pre[4][GA_WORDS];
    const u32 w = wave_id(), lane = lane_id();
    const u32 t = blockIdx.x * 4 + w;
    if (t >= nt) return;
    const u32 c = blk_cnt[t] & 0xffffu;
    if (c == 0) return;
    const u32 e0 = tiles[t].e0;
    const u64 d = dst_off[t] & 0xffffffffull;      // (the high word counts finished suffixes: InBlkCnt)
    u32 *occ = s_occ[w], *head = s_head[w], *pre = s_pre[w];
    for (u32 i = lane; i < GA_WORDS; i += kWave) occ[i] = head[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (u32 i = lane; i < c; i += kWave) {
        const u32 q = st_pos[e0 + i] - e0;
        atomicOr(&occ[q >> 5], 1u << (q & 31u));
        if (!(st_idx[e0 + i] >> 31)) atomicOr(&head[q >> 5], 1u << (q & 31u));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    {   // exclusive prefix of the popcounts: four consecutive words per lane
        const u32 c0 = __popc(occ[4 * lane]), c1 = __popc(occ[4 * lane + 1]), c2 = __popc(occ[4 * lane + 2]),
                  c3 = __popc(occ[4 * lane + 3]);
        const u32 ex = wave_incl_sum(c0 + c1 + c2 + c3) - (c0 + c1 + c2 + c3);
        pre[4 * lane] = ex;
        pre[4 * lane + 1] = ex + c0;
        pre[4 * lane + 2] = ex + c0 + c1;
        pre[4 * lane + 3] = ex + c0 + c1 + c2;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (u32 i = lane; i < c; i += kWave) {
        const u32 ps = st_pos[e0 + i], q = ps - e0;
        const u32 below = (q & 31u) ? (occ[q >> 5] & ((1u << (q & 31u)) - 1u)) : 0u;
        const u32 rank = pre[q >> 5] + __popc(below);
        // nearest head at or below q (exists: the first element of a group is never flagged)
        u32 wi = q >> 5;
        u32 m = head[wi] & ((q & 31u) == 31u ? ~0u : ((2u << (q & 31u)) - 1u));
        while (m == 0 && wi > 0) m = head[--wi];
        const u32 hq = wi * 32 + (31u - (u32)__builtin_clz(m | 1u));
        pos[d + rank] = ps;
        idx[d + rank] = st_idx[e0 + i] & 0x7fffffffu;
        grp[d + rank] = e0 + hq + 1;
    }
}

// ---- finishing small groups ----------------------------------------------------------------------

// Nearly every tied group the local sort leaves on log-like text is a pair or a triple that differs within the next few
// symbols.  The rounds of sa_build.hip would resolve them with their general machinery -- some twenty launches and a host
// round trip for a few megabytes of data.  This kernel runs between the local sort and the gather instead and settles
// such groups where they lie: one wavefront per tile block (the same unit as the gather: a tile holds a few dozen
// records), the head of every group of g <= FIN_MAX members packs ONE more 64-bit text key per member (text_key_at from
// symbol h0 on: the packing of the text rounds), and when the g keys are pairwise different writes the members to
// sa_out[head slot + number of smaller keys].  Such a group's records are dropped; every other group (larger, or two
// equal keys) keeps ALL its records, untouched.  The leftovers are compacted inside the block, blk_cnt[t] is updated (what
// is left, and in its high half what was dropped: InBlkCnt), and the scan and msd_gather_kernel build the active list from
// them as before.
// FIN_MAX: the ranking is all-pairs, in registers.  The 2^29-byte `lines` chunk leaves 1 044 432 pairs and 1 396 triples
// (random text: groups of four are expected a handful of times per chunk, of five once in hundreds of chunks), and a group
// left behind costs the whole tail of launches again.
constexpr int FIN_MAX = MSD_FIN_MAX;
constexpr u32 FIN_WORDS = GA_WORDS + 2;      // the bitmap of flagged slots, read 64 bits at a time from any slot + 1 of the tile
struct MsdFinish {
    const u8 *codes;
    int code_bits, key_syms, plus_one;       // key_syms = min(64 / code_bits, 16)
    u32 h0, n;                               // whole symbols the sort key has compared
};

__global__ __launch_bounds__(256) void msd_finish_kernel(const MsdTile *tiles, u32 *blk_cnt, u32 nt, u32 *st_pos, u32 *st_idx,
                                                           u32 *sa_out, MsdFinish f)
{
    __shared__ u32 s_tie[4][FIN_WORDS], s_done[4][GA_WORDS];
    const u32 w = wave_id(), lane = lane_id();
    const u32 t = blockIdx.x * 4 + w;
    if (t >= nt) return;
    // The kernel is a chain of dependent trips to memory (count and tile -> records -> the members' suffixes -> their
    // text), a hundred thousand waves of it: the two first loads go out together, and the first 64 records of the block
    // (a tile of `lines` has 32 on average, 77 at most) stay in registers for all three passes over them.
    const u32 c = blk_cnt[t] & 0xffffu;
    const u32 e0 = tiles[t].e0;
    if (c == 0) return;
    u32 ps0 = 0, v0 = 0;
    if (lane < c) {
        ps0 = st_pos[e0 + lane];
        v0 = st_idx[e0 + lane];
    }
    auto record = [&](u32 i, u32 &ps, u32 &v) {
        if (i < (u32)kWave) {
            ps = ps0;
            v = v0;
        } else {
            ps = st_pos[e0 + i];
            v = st_idx[e0 + i];
        }
    };
    u32 *tie = s_tie[w], *done = s_done[w];
    for (u32 i = lane; i < FIN_WORDS; i += kWave) tie[i] = 0;
    for (u32 i = lane; i < GA_WORDS; i += kWave) done[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (u32 i = lane; i < c; i += kWave) {
        u32 ps, v;
        record(i, ps, v);
        const u32 q = ps - e0;
        if (v >> 31) atomicOr(&tie[q >> 5], 1u << (q & 31u));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    bool settled = false;
    for (u32 i = lane; i < c; i += kWave) {
        u32 ps, v;
        record(i, ps, v);
        if (v >> 31) continue;               // (a group is handled by its head: the one member without the flag)
        const u32 q = ps - e0, a = q + 1u;
        // members = the flagged slots that follow the head without a gap
        const u64 win = (((u64)tie[(a >> 5) + 1u] << 32) | (u64)tie[a >> 5]) >> (a & 31u);
        const u32 g = win == ~0ull ? 65u : 1u + (u32)__builtin_ctzll(~win);
        if (g > (u32)FIN_MAX) continue;
        u32 sfx[FIN_MAX], rk[FIN_MAX];
        u64 key[FIN_MAX];
#pragma unroll
        for (int j = 0; j < FIN_MAX; ++j) {
            sfx[j] = 0;
            key[j] = 0;
            rk[j] = 0;
            if ((u32)j < g) {
                sfx[j] = j == 0 ? v : sa_out[ps + j];
                const u64 at = (u64)sfx[j] + f.h0;
                if (at < f.n) key[j] = text_key_at(f.codes, (u32)at, f.code_bits, f.key_syms, f.plus_one, f.n);
            }
        }
        bool same = false;
#pragma unroll
        for (int j = 0; j < FIN_MAX; ++j) {
#pragma unroll
            for (int l = j + 1; l < FIN_MAX; ++l) {
                if ((u32)l < g) {
                    same |= key[j] == key[l];
                    rk[l] += key[j] < key[l] ? 1u : 0u;
                    rk[j] += key[j] < key[l] ? 0u : 1u;
                }
            }
        }
        if (same) continue;
        settled = true;
#pragma unroll
        for (int j = 0; j < FIN_MAX; ++j) {
            if ((u32)j < g) {
                sa_out[ps + rk[j]] = sfx[j];
                atomicOr(&done[(q + j) >> 5], 1u << ((q + j) & 31u));
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (__ballot(settled) == 0) return;      // nothing dropped: the block stays as it is
    // the records of the groups that stay, packed to the front of the block (a record moves down or stays: the 64 records
    // of a trip are read before any of them is written, and what they overwrite was read in this trip or an earlier one)
    u32 kept = 0;
    for (u32 base = 0; base < c; base += kWave) {
        const u32 i = base + lane;
        u32 ps = 0, v = 0;
        bool keep = false;
        if (i < c) {
            record(i, ps, v);
            const u32 q = ps - e0;
            keep = ((done[q >> 5] >> (q & 31u)) & 1u) == 0;
        }
        const u64 km = __ballot(keep);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (keep) {
            const u32 o = e0 + kept + mbcnt(km);
            st_pos[o] = ps;
            st_idx[o] = v;
        }
        kept += (u32)__popcll(km);
    }
    if (lane == 0) blk_cnt[t] = kept | ((c - kept) << 16);      // (InBlkCnt)
}

// ---- local sort --------------------------------------------------------------------------------

// One workgroup per tile: <= 8192 elements of <= 1024 consecutive joint buckets.  Sort key in LDS:
// [ bucket number inside the tile | remaining key bits | suffix index ] -- stable 8-bit LSD passes
// over the bucket and key bits (the index bits ride along), wave-ballot ranking as in radix_sort.hip.
// This is the general (slower) form: it takes whatever the fast kernel below hands back.
__global__ __launch_bounds__(MSD_BLOCK) void msd_local_sort_kernel(const u64 *in, const MsdTile *tiles, int rem_bits, int idx_bits,
                                                                     u32 *sa_out, const u32 *tile_list, int fused, MsdEmit em_val)
{
    const MsdEmit *em = fused ? &em_val : nullptr;
    __shared__ __attribute__((aligned(16))) u64 exch[MSD_TILE];
    __shared__ u32 wave_hist[MSD_WAVES][256];
    __shared__ u32 scr[MSD_WAVES + 1];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 t = tile_list ? tile_list[blockIdx.x] : blockIdx.x;
    const MsdTile td = tiles[t];
    const u32 e0 = td.e0, count = td.count;
    for (u32 i = tid; i < MSD_WAVES * 256; i += MSD_BLOCK) (&wave_hist[0][0])[i] = 0;
    __syncthreads();
    int seg_bits = 0;
    while ((1u << seg_bits) < td.nb) ++seg_bits;
    const u64 tag_base = (u64)td.tag0 << (rem_bits + idx_bits);
    // element r of this thread sits at tile position wave * 1024 + r * 64 + lane (order = position)
    u64 key[MSD_IPT];
#pragma unroll
    for (int r = 0; r < MSD_IPT; ++r) {
        const u32 p = wave * (kWave * MSD_IPT) + r * kWave + lane;
        // [bucket inside the tile | remaining key bits | index] (G2 tagged the element with its bucket's number); ~0: padding
        key[r] = p < count ? in[e0 + p] - tag_base : ~0ull;
    }
    const int sort_bits = rem_bits + seg_bits;
    for (int shift = idx_bits; shift < idx_bits + sort_bits; shift += 8) {
        const int left = idx_bits + sort_bits - shift;
        const u32 dmask = left >= 8 ? 0xffu : ((1u << left) - 1u);
        u32 rank[MSD_IPT], prev[MSD_IPT];
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) {
            // padding (positions >= count) carries the largest digit of every pass: a stable sort keeps it last
            const bool pad = wave * (kWave * MSD_IPT) + r * kWave + lane >= count;
            const u32 d = pad ? dmask : ((u32)(key[r] >> shift) & dmask);
            const u64 peers = match_digit8(d, ~0ull);
            const u32 below = mbcnt(peers);
            prev[r] = 0;
            if (below == 0) prev[r] = atomicAdd(&wave_hist[wave][d], (u32)__popcll(peers));
            rank[r] = below | ((u32)__builtin_ctzll(peers) << 16);
        }
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) rank[r] = __shfl(prev[r], (int)(rank[r] >> 16)) + (rank[r] & 0xffffu);
        __syncthreads();
        {
            // digit d is owned by thread d (the first four waves); exclusive prefix over the 256 digits
            u32 c[MSD_WAVES];
            u32 total = 0;
            if (tid < 256) {
#pragma unroll
                for (int w = 0; w < MSD_WAVES; ++w) {
                    c[w] = wave_hist[w][tid];
                    total += c[w];
                }
            }
            const u32 incl = wave_incl_sum(total);
            if (lane == kWave - 1) scr[wave] = incl;
            __syncthreads();
            if (tid < 256) {
                u32 run = incl - total;
                for (u32 w = 0; w < wave; ++w) run += scr[w];
#pragma unroll
                for (int w = 0; w < MSD_WAVES; ++w) {
                    wave_hist[w][tid] = run;
                    run += c[w];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) {
            const bool pad = wave * (kWave * MSD_IPT) + r * kWave + lane >= count;
            const u32 d = pad ? dmask : ((u32)(key[r] >> shift) & dmask);
            exch[wave_hist[wave][d] + rank[r]] = key[r];
        }
        __syncthreads();
        for (u32 i = tid; i < MSD_WAVES * 256; i += MSD_BLOCK) (&wave_hist[0][0])[i] = 0;
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) key[r] = exch[wave * (kWave * MSD_IPT) + r * kWave + lane];
        __syncthreads();
    }
    if (sort_bits <= 0) {            // nothing to sort (one bucket, no key bits left): still goes through LDS for the flags
#pragma unroll
        for (int r = 0; r < MSD_IPT; ++r) exch[wave * (kWave * MSD_IPT) + r * kWave + lane] = key[r];
        __syncthreads();
    }
    if (tid == 0) scr[0] = 0;
    __syncthreads();
    msd_emit_tile(exch, count, e0, idx_bits, sa_out, em, &scr[0]);
    __syncthreads();
    if (em && tid == 0) em->blk_cnt[t] = scr[0];
}


// The fast form.  One counting pass on the top 13 bits of (bucket, key) with returning LDS atomics (no
// order to preserve: the whole element, index included, is the sort key, so the result is a total order
// anyway) leaves bins of a handful of elements; every element then finds its place inside its bin by
// counting the smaller ones -- neighbouring lanes sit in the same bin, so those LDS reads are broadcasts.
// A tile with more than LS_KMAX elements under one value of the top LS_DECLINE_BITS bits (many equal or
// nearly equal keys) is handed to the general kernel instead.
//
// ONE array of counters: counts, scanned in place to the bins' starts; the slot atomics then run every start up
// to its bin's end, which is the next bin's start whether or not either is empty -- the ranking reads the start
// of bin b from entry b - 1, and a zero halfword in front of the array (the top of the tile's last, never used
// slot) serves bin 0.  That leaves the 16 KiB behind the tile to 8192 bins instead of 4096 and their copy.
#ifndef PSS_LS_BIN_BITS
#define PSS_LS_BIN_BITS 13
#endif
constexpr int LS_BIN_BITS = PSS_LS_BIN_BITS;
constexpr u32 LS_BINS = 1u << LS_BIN_BITS;          // 16-bit counters, two per LDS word (a tile has < 8192 elements)
constexpr u32 LS_WORDS = LS_BINS / 2;
constexpr u32 LS_KMAX = 64;
constexpr int LS_DECLINE_BITS = 12;                 // the decline rule does not move with the bins: msd_slow_tiles is observable
static_assert(LS_BIN_BITS >= LS_DECLINE_BITS && LS_BIN_BITS <= 13, "the counters fill the 16 KiB behind the tile at most");
#ifndef PSS_LS_GROUP
#define PSS_LS_GROUP 1
#endif
constexpr int LS_GROUP = PSS_LS_GROUP;              // rows ranked / written out together: their LDS reads are issued back to back
#ifndef PSS_LS_SLOT_GROUP
#define PSS_LS_SLOT_GROUP 1
#endif
constexpr int LS_SLOT_GROUP = PSS_LS_SLOT_GROUP;    // rows whose slot atomics are in flight together
#ifndef PSS_LS_WINDOW
#define PSS_LS_WINDOW 7
#endif
// Members of its bin every element reads unconditionally.  A knob of the ranking alone (the tile plan reserves eight
// sentinel slots whatever it is).  What counts is the share of WAVES with a lane in a longer bin, which all run the
// divergent loop: on the bench text (39 symbols in 6-bit codes: most bin numbers cannot occur) an element of a
// two-bucket tile sees its bin 3.1 long on average at 8192 bins -- tests/tools/local_bins_model.py, DESIGN §4.2.
constexpr int LS_WINDOW = PSS_LS_WINDOW;
static_assert(LS_WINDOW >= 1 && LS_WINDOW <= 8 && MSD_TILE_CAP + 8 + 8 <= MSD_TILE, "the sentinels end before the scalars");
static_assert((LS_KMAX >> (LS_BIN_BITS - LS_DECLINE_BITS)) >= (u32)LS_WINDOW, "bins that are declined together: one of them outgrows the window");

__global__ __launch_bounds__(256) void msd_tile_desc_kernel(const u32 *cstart, const u32 *tile_first, u32 nt, u32 ne, u32 n,
                                                              MsdTile *tiles, const u32 *cj, const u64 *ntp, const u64 *nep)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (ntp) {                     // (counts on the device: see InTileHeadDev)
        nt = (u32)*ntp;
        ne = (u32)*nep;
    }
    if (t >= nt) return;
    const u32 k0 = tile_first[t], k1 = tile_first[t + 1];
    const u32 e0 = cstart[k0], e1 = k1 < ne ? cstart[k1] : n;
    if (cj) {
        // LSD order: the tag is the joint bucket number mod 64, the tile lies inside one block of 64: "buckets" = the span of
        // its tags (a joint bucket that is empty between two of them just takes a number)
        const u32 t0 = cj[k0] & (MSD_RAW_TAG_SPAN - 1u), t1 = cj[k1 - 1] & (MSD_RAW_TAG_SPAN - 1u);
        tiles[t] = MsdTile{e0, e1 - e0, t0, t1 - t0 + 1u};
    } else {
        tiles[t] = MsdTile{e0, e1 - e0, k0 & (MSD_TAG_SPAN - 1u), k1 - k0};
    }
}

// The rows of a tile (row r = positions r * 512 + tid), G at a time: every row but the last one is full, so a group
// that ends before the last row runs f(true, g) with no lane predicate at all, under a scalar branch; the group that
// holds the last row runs f(false, g), the one body that tests p < count.
template <int G, class F>
__device__ __forceinline__ void ls_rows(u32 rows, F &&f)
{
    static_assert(MSD_IPT % G == 0, "the groups tile the rows");
    // (every phase compares the row count anew, a scalar compare and branch per group: shared between the phases, the
    // sixteen outcomes are sixteen lane masks alive for the whole tile)
    rows = (u32)__builtin_amdgcn_readfirstlane((int)rows);
    asm volatile("" : "+s"(rows));
#pragma unroll
    for (int g = 0; g < MSD_IPT; g += G) {
        // (two tests of their own, not if / else: each stays a scalar compare and branch)
        if ((u32)(g + G) < rows) {
            f(std::true_type{}, g);
            asm volatile("");      // (keeps the two bodies apart: merged, every row is back under a lane mask)
        }
        if (rows - 1u - (u32)g < (u32)G) {
            asm volatile("");      // (or this test is folded into the tail's lane mask, and every row computes one)
            f(std::false_type{}, g);
        }
    }
}

// A tile lives ~3 us, and what it needs first -- its descriptor, then the starts of its buckets and its
// elements -- are dependent trips to HBM of ~1 us each: one workgroup per tile leaves the CU waiting for
// memory most of the time.  The workgroups therefore persist (two per CU) and walk over the tiles with the
// loads one tile ahead: descriptor two tiles ahead, bucket starts and elements of the next tile issued as
// soon as the registers of the current one are free, landing while the current tile is being sorted.
// nt_dev (optional): the number of tiles is read on the device, and the kernel does nothing when the plan it would run on
// is not to be used -- a bucket beyond a tile (counters[1]) or a byte without a code (*bad_dev): the host learns both after
// the launch, in the one round trip of the sort.
__global__ __launch_bounds__(MSD_BLOCK, 4) void msd_local_fast_kernel(const u64 *in, const MsdTile *tiles, u32 nt, int rem_bits,
                                                                     int idx_bits, u32 *sa_out, u32 *fail_list, u32 *fail_count,
                                                                     int fused, MsdEmit em_val, const u64 *nt_dev,
                                                                     const u32 *counters_dev, const u32 *bad_dev)
{
    if (nt_dev) {
        if (counters_dev[1] > MSD_MAX_BUCKET || (bad_dev && *bad_dev)) return;
        nt = (u32)*nt_dev;
    }
    const MsdEmit *em = fused ? &em_val : nullptr;
    // 80 KiB of LDS to the byte: two workgroups per CU.  One array: the tile, then the counters -- the ranking below reads
    // up to LS_WINDOW - 1 elements past the tile's last slot (masked out afterwards), and those reads must stay inside it.
    __shared__ __attribute__((aligned(16))) u64 lds_all[MSD_TILE + LS_WORDS / 2];
    u64 *const exch = lds_all;
    u32 *const hist = reinterpret_cast<u32 *>(lds_all + MSD_TILE);      // counts, then bin starts, then (after the slot atomics) bin ends, packed
    u32 *const scr = reinterpret_cast<u32 *>(&exch[MSD_TILE - 8]);      // a tile never reaches these slots (MSD_MAX_BUCKET)
    u32 &s_fail = scr[MSD_WAVES + 2];
    // scr[0 .. 11] are in use; scr[15], the word in front of the counters, stays zero: "the end of bin -1"
    static_assert(MSD_WAVES + 3 < 15, "the word in front of the counters is nobody's");
    u32 tid = threadIdx.x;
    const u32 stride = gridDim.x;
    u32 t = blockIdx.x;
    if (t >= nt) return;
    MsdTile cur = tiles[t];
    MsdTile nxt = t + stride < nt ? tiles[t + stride] : MsdTile{0, 0, 0, 0};
    u64 pe[MSD_IPT];          // prefetched raw elements of the tile about to be sorted (rows beyond the tile: left as they are)
    auto prefetch = [&](const MsdTile &d) {
        const u64 *const src = in + d.e0;
        ls_rows<1>((d.count + MSD_BLOCK - 1) / MSD_BLOCK, [&](auto full, int r) __attribute__((always_inline)) {
            const u32 p = r * MSD_BLOCK + tid;
            if (decltype(full)::value || p < d.count) pe[r] = src[p];
        });
    };
    prefetch(cur);
    // Six barriers per tile, not nine: the counters are zeroed for the NEXT tile while this one is permuted (they are not
    // read after the ranking), the tile's bookkeeping (failure flag, record count -> blk_cnt) is settled behind the next
    // tile's first barrier -- by then every wave has left this tile's output -- and nothing separates the tiles otherwise
    // (the next write to the element array is three barriers into the next tile).
    for (u32 i = tid; i < LS_WORDS; i += MSD_BLOCK) hist[i] = 0;
    if (tid == 0) {
        s_fail = 0;
        scr[MSD_WAVES + 3] = 0;            // records the tile has emitted
        scr[15] = 0;                       // bin 0 starts at 0, for every tile: nothing else writes here
    }
    lds_barrier();
    u32 prev_t = 0;
    bool prev_ok = false;
    for (;;) {
        const u32 count = cur.count, e0 = cur.e0;
        const u32 rows = (count + MSD_BLOCK - 1) / MSD_BLOCK;          // uniform over the workgroup
        int seg_bits = 0;
        while ((1u << seg_bits) < cur.nb) ++seg_bits;
        const u64 tag_base = (u64)cur.tag0 << (rem_bits + idx_bits);
        const int sort_bits = rem_bits + seg_bits;
        const int bin_shift = idx_bits + (sort_bits > LS_BIN_BITS ? sort_bits - LS_BIN_BITS : 0);
        // Nothing derived from the thread number is carried from tile to tile: hoisted out of this loop, the lane masks
        // and addresses of every phase outgrow the scalar registers and come back as lane moves in every row.
        asm volatile("" : "+v"(tid));
        const u32 wave_no = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));      // this wave's number, as a scalar
        u64 e[MSD_IPT];
        ls_rows<1>(rows, [&](auto full, int r) __attribute__((always_inline)) {
            if (decltype(full)::value || r * MSD_BLOCK + tid < count) {
                // the element carries its bucket (G2 put it there): [bucket inside the tile | remaining key bits | index]
                e[r] = pe[r] - tag_base;
                const u32 bin = (u32)(e[r] >> bin_shift);
                atomicAdd(&hist[bin >> 1], 1u << (16u * (bin & 1u)));    // count now; the slot is taken after the scan
            }
        });
        // the raw elements are consumed: their registers take the next tile while this one is sorted (past the last
        // tile `nxt` is empty: no rows, no loads)
        const bool more = t + stride < nt;
        prefetch(nxt);
        lds_barrier();
        if (tid == 0) {                    // the previous tile is over for every wave: its record count, the flags for this one
            if (em && prev_ok) em->blk_cnt[prev_t] = scr[MSD_WAVES + 3];
            s_fail = 0;
            scr[MSD_WAVES + 3] = 0;
        }
        {
            // exclusive scan over the bins in place: LS_WPT adjacent words = 2 LS_WPT bins per thread (eight words at 8192 bins)
            constexpr int LS_WPT = LS_WORDS / MSD_BLOCK;
            static_assert(LS_WPT * MSD_BLOCK == (int)LS_WORDS && LS_WPT >= 1, "bins split evenly over the threads");
            u32 c[2 * LS_WPT];
            u32 sum = 0;
#pragma unroll
            for (int j = 0; j < LS_WPT; ++j) {
                const u32 wv = hist[LS_WPT * tid + j];
                c[2 * j] = wv & 0xffffu;
                c[2 * j + 1] = wv >> 16;
                sum += c[2 * j] + c[2 * j + 1];
            }
            const u32 incl = wave_incl_sum_dpp(sum);
            if ((tid & (kWave - 1u)) == kWave - 1u) scr[wave_no] = incl;
            lds_barrier();
            // the totals of the waves before mine: all eight read at once, chosen by the (scalar) wave number
            static_assert(MSD_WAVES == 8, "two 16-byte reads hold the totals of all waves");
            const uint4 w03 = *reinterpret_cast<const uint4 *>(&scr[0]), w47 = *reinterpret_cast<const uint4 *>(&scr[4]);
            const u32 wtot[MSD_WAVES] = {w03.x, w03.y, w03.z, w03.w, w47.x, w47.y, w47.z, w47.w};
            u32 ex = incl - sum;
#pragma unroll
            for (u32 w = 0; w + 1 < (u32)MSD_WAVES; ++w) ex += w < wave_no ? wtot[w] : 0u;
#pragma unroll
            for (int j = 0; j < LS_WPT; ++j) {
                const u32 lo = ex, hi = ex + c[2 * j];
                hist[LS_WPT * tid + j] = lo | (hi << 16);
                ex = hi + c[2 * j + 1];
            }
        }
        lds_barrier();
        // (a second returning atomic on the bin's start hands out the slot: one more LDS atomic per element, sixteen
        // fewer registers held across the prefetch; when all have theirs, the word holds the bin's END).  LS_SLOT_GROUP
        // rows have their atomics in flight together before the first of them is waited for.
        ls_rows<LS_SLOT_GROUP>(rows, [&](auto full, int g) __attribute__((always_inline)) {
            u32 slot[LS_SLOT_GROUP], sh[LS_SLOT_GROUP];
#pragma unroll
            for (int j = 0; j < LS_SLOT_GROUP; ++j) {
                if (decltype(full)::value || (g + j) * MSD_BLOCK + tid < count) {
                    const u32 bin = (u32)(e[g + j] >> bin_shift);
                    sh[j] = 16u * (bin & 1u);
                    slot[j] = atomicAdd(&hist[bin >> 1], 1u << sh[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < LS_SLOT_GROUP; ++j) {
                if (decltype(full)::value || (g + j) * MSD_BLOCK + tid < count) exch[(slot[j] >> sh[j]) & 0xffffu] = e[g + j];
            }
        });
        // sentinels behind the tile, as many as the window is wide: the ranking window of the last bins reads them
        // (count + LS_WINDOW - 1 < the scalars' slots: MSD_TILE_CAP)
        if (tid < (u32)LS_WINDOW) exch[count + tid] = ~0ull;
        lds_barrier();
        // Place inside the bin = number of smaller elements there (thread <-> position: neighbours share the bin, their
        // reads are broadcasts).  The kernel is bound by the latency of dependent LDS reads, not by their number: every
        // element reads a fixed window of LS_WINDOW members of its bin (no loop, no branch -- a read past the bin is
        // masked out), LS_GROUP rows at a time with all their reads in flight; a longer bin finishes in a loop that the
        // whole wave waits for (how many waves have one: the comment at LS_WINDOW).
        // starts16[bin] = the end of bin - 1 = first slot of the bin, starts16[bin + 1] = first slot behind it; starts16[0] is
        // the zero halfword in front of the counters
        const u16 *const starts16 = reinterpret_cast<const u16 *>(hist) - 1;
        // bins that share their top LS_DECLINE_BITS bits: 2^pair_bits neighbours (one where the key is no wider than that)
        const int pair_bits = (sort_bits > LS_DECLINE_BITS ? sort_bits - LS_DECLINE_BITS : 0) - (sort_bits > LS_BIN_BITS ? sort_bits - LS_BIN_BITS : 0);
        u32 rk[MSD_IPT];
        u32 rank_rows = (u32)__builtin_amdgcn_readfirstlane((int)rows);
        asm volatile("" : "+s"(rank_rows));      // (as in ls_rows)
#pragma unroll
        for (int g = 0; g < MSD_IPT; g += LS_GROUP) {
            if ((u32)g < rank_rows) {
                u64 x[LS_GROUP];
                u32 s0[LS_GROUP], sm[LS_GROUP];
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) x[j] = exch[(g + j) * MSD_BLOCK + tid];
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    const u32 bin = (u32)(x[j] >> bin_shift) & (LS_BINS - 1u);      // (a slot past the tile holds anything)
                    s0[j] = starts16[bin];
                }
                u64 y[LS_GROUP][LS_WINDOW];
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
#pragma unroll
                    for (int k = 0; k < LS_WINDOW; ++k) y[j][k] = exch[s0[j] + k];
                }
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    u32 c = 0;
#pragma unroll
                    for (int k = 0; k < LS_WINDOW; ++k) {
                        keep_load(y[j][k]);      // (or the compiler makes every read conditional on k < len: a branch and a wait per read)
                        // (no "k < len": what lies behind my bin in the window belongs to LATER bins -- larger numbers, the
                        // elements being in bin order -- or is a sentinel; eight compares and eight mask operations fewer per element)
                        c += y[j][k] < x[j] ? 1u : 0u;
                    }
                    sm[j] = c;
                }
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    // the window's last member still in my bin: the bin may go on -- only then is its length looked up, and
                    // that of the bins it shares its top LS_DECLINE_BITS bits with: more than LS_KMAX there decline the
                    // tile (such a group has a bin longer than the window, so some lane gets here)
                    // (no lane predicate on the row: a lane past the tile ranks whatever its slot holds, and is asked
                    // p < count only in here)
                    if (((y[j][LS_WINDOW - 1] ^ x[j]) >> bin_shift) == 0 && (g + j) * MSD_BLOCK + tid < count) {
                        const u32 bin = (u32)(x[j] >> bin_shift) & (LS_BINS - 1u);
                        const u32 len = (u32)starts16[bin + 1u] - s0[j];
                        const u32 lo = bin >> pair_bits << pair_bits;
                        if ((u32)starts16[lo + (1u << pair_bits)] - (u32)starts16[lo] > LS_KMAX) {
                            s_fail = 1;
                        } else {
                            for (u32 q = s0[j] + LS_WINDOW; q < s0[j] + len; ++q) sm[j] += exch[q] < x[j] ? 1u : 0u;
                        }
                    }
                    e[g + j] = x[j];
                    rk[g + j] = s0[j] + sm[j];
                }
            }
        }
        lds_barrier();
        const bool failed = s_fail != 0;
        if (failed) {
            if (tid == 0) fail_list[atomicAdd(fail_count, 1u)] = t;
        } else {
            ls_rows<1>(rows, [&](auto full, int r) __attribute__((always_inline)) {
                if (decltype(full)::value || r * MSD_BLOCK + tid < count) exch[rk[r]] = e[r];
            });
        }
        for (u32 i = tid; i < LS_WORDS; i += MSD_BLOCK) hist[i] = 0;      // (bin starts: last read in the ranking) for the next tile
        lds_barrier();
        if (!failed) {
            // Output, LS_GROUP rows with their loads in flight: suffix indices to sa_out[e0 ..], bit 31 = "same key as my
            // predecessor" unless the first rerank is fused.  Fused, the array is written clean and a row only notes its two
            // tie bits (bit r: row r owes a record -- it or its successor is tied --, bit 16 + r: tied with its predecessor);
            // the records go out behind the rows.  One address per tile for the tile and one for the array: rows are a
            // constant apart.
            const u32 imask = (u32)((1ull << idx_bits) - 1ull);
            const u32 flag = em == nullptr ? 0x80000000u : 0u;
            const u64 same = 1ull << idx_bits;
            const u64 *const my = exch + tid;
            u32 *const out = sa_out + e0 + tid;
            u32 ties = 0;
            ls_rows<LS_GROUP>(rows, [&](auto full, int g) __attribute__((always_inline)) {
                u64 cur[LS_GROUP], prv[LS_GROUP], nxt[LS_GROUP];
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    const int o = (g + j) * MSD_BLOCK;
                    cur[j] = my[o];
                    prv[j] = o == 0 ? exch[tid - (tid != 0 ? 1u : 0u)] : my[o - 1];      // (position 0 has no predecessor: below)
                    nxt[j] = my[o + 1];                                                 // (position 8191 + 1 is the first counter word)
                }
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    keep_load(cur[j]);
                    keep_load(prv[j]);
                    keep_load(nxt[j]);
                }
#pragma unroll
                for (int j = 0; j < LS_GROUP; ++j) {
                    const int o = (g + j) * MSD_BLOCK;
                    bool tie = (prv[j] ^ cur[j]) < same;      // equal above the index bits
                    if (o == 0) tie = tie && tid != 0;
                    // a full row has a successor inside the tile at every position (the last row is not empty)
                    const bool tie_next = (nxt[j] ^ cur[j]) < same && (decltype(full)::value || o + tid + 1u < count);
                    if (decltype(full)::value || o + tid < count) {
                        out[o] = ((u32)cur[j] & imask) | (tie ? flag : 0u);
                        ties |= ((tie || tie_next) ? 1u << (g + j) : 0u) | (tie ? 0x10000u << (g + j) : 0u);
                    }
                }
            });
            if (em != nullptr) {
                // the records of the few tied elements (0.4 % of natural text): a wave without any skips the loop
                u32 *const s_count = &scr[MSD_WAVES + 3];
                for (u32 m = ties & 0xffffu; m != 0; m &= m - 1u) {
                    const u32 r = (u32)__builtin_ctz(m);
                    const u32 p = r * MSD_BLOCK + tid;
                    const u32 slot = e0 + atomicAdd(s_count, 1u);
                    em->st_pos[slot] = e0 + p;
                    em->st_idx[slot] = ((u32)exch[p] & imask) | ((ties >> (16u + r)) << 31);
                }
            }
        }
        prev_t = t;
        prev_ok = !failed;
        if (!more) break;
        t += stride;
        cur = nxt;
        nxt = t + stride < nt ? tiles[t + stride] : MsdTile{0, 0, 0, 0};
    }
    if (em) {
        lds_barrier();
        if (tid == 0 && prev_ok) em->blk_cnt[prev_t] = scr[MSD_WAVES + 3];
    }
}

#include "ss_sort_impl.h"

#include "msd_driver_impl.h"

}  // namespace pss
