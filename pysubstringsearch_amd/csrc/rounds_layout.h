// rounds_layout.h -- what the host driver of the rounds (sa_refine_impl.h, anchor_driver_impl.h) and the kernels of
// sa_rounds_impl.h / anchor_impl.h have to agree on: the tile constants and the rows of their tables, ONE description of
// every scratch slot the rounds carve (offsets of the regions and an end, functions of the sizes alone), and the rules
// the driver decides by, as pure functions of their arguments.  Plain C++ without HIP, like msd_layout.h and
// build_plan.h: everything here is arithmetic (tests/native/rounds_layout.cpp restates it on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

namespace pss {

// ---- constants and rows the kernels share with the layouts ---------------------------------------------------------

constexpr int GS_T = 2048;      // elements per workgroup window
#ifndef PSS_GS_CAP
#define PSS_GS_CAP 512
#endif
constexpr int GS_CAP = PSS_GS_CAP;     // largest group ranked in LDS (= halo on both sides)
constexpr uint32_t MID_CAP = 4096;     // largest group of the middle tier (one workgroup, in LDS)
#ifndef PSS_MID_KMAX
#define PSS_MID_KMAX 512
#endif
constexpr uint32_t MID_KMAX = PSS_MID_KMAX;
struct MidGroup {
    uint32_t start, size;
};
constexpr uint32_t BG_TILE = 4096;     // elements of a tile of the segmented merge sort
struct BigTile {
    uint32_t gstart, gsize, t;      // tile t of the group whose members are [gstart, gstart + gsize) of the compacted list
};
constexpr uint32_t ANC_TILE = 4096;        // window starts per workgroup pass (256 threads x 16)
constexpr uint32_t ROUNDS_SCAN_BLOCKS = 1024;      // SC_MAX_BLOCKS of scan.h (which needs HIP): partial sums of a device_excl_scan

namespace rounds_detail {
inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// Regions one behind the other, every start on a multiple of `align`.
struct Carver {
    size_t o = 0, align;
    explicit Carver(size_t a) : align(a) {}
    size_t operator()(size_t bytes)
    {
        const size_t at = o;
        o = up(o + bytes, align);
        return at;
    }
};
}  // namespace rounds_detail

// ---- the scratch slots ---------------------------------------------------------------------------------------------
// Members are byte offsets from the slot's base; `end` is the offset behind the last region, reserved() what the driver
// asks the slot for (never less than `end`: the native test walks the sizes).

// Slot S_SCR, one group-local round over m elements: the large-group flags, the per-window tallies and their scans, and
// with the middle tier its two group lists and their two counters.
struct RoundScratch {
    uint32_t nblk;              // windows of GS_T elements
    size_t big, blk_big, blk_heads, off_big, off_heads, partial, mid = 0, mid_fail = 0, mid_count = 0, end;
    static constexpr size_t TOTAL_AT = ROUNDS_SCAN_BLOCKS;      // the scans' total, behind the partial sums
    RoundScratch(uint32_t m, bool mid_tier) : nblk((uint32_t)(((uint64_t)m + GS_T - 1) / GS_T))
    {
        rounds_detail::Carver carve(64);
        big = carve(m);
        blk_big = carve((size_t)nblk * 4);
        blk_heads = carve((size_t)nblk * 4);
        off_big = carve(((size_t)nblk + 1) * 8);
        off_heads = carve(((size_t)nblk + 1) * 8);
        partial = carve((ROUNDS_SCAN_BLOCKS + 2) * 8);
        if (mid_tier) {
            mid = carve(((size_t)m / 2 + 16) * sizeof(MidGroup));
            mid_fail = carve(((size_t)m / 512 + 16) * sizeof(MidGroup));      // (groups of > 512 members)
            mid_count = carve(64);
        }
        end = carve.o;
    }
    // (with or without the middle tier: the slot does not shrink when a switch is thrown)
    static size_t reserved(uint32_t m)
    {
        const size_t nblk = ((size_t)m + GS_T - 1) / GS_T;
        return (size_t)m + nblk * 24 + (ROUNDS_SCAN_BLOCKS + 8) * 8 + 4096 + ((size_t)m / 2 + 16) * sizeof(MidGroup) +
               ((size_t)m / 512 + 16) * sizeof(MidGroup) + 512;
    }
};

// Slot S_BIG: the nbig members of the large groups, compacted -- their places in the list, their dense group numbers,
// and the two (key, value) buffers their sort goes back and forth between.
struct BigScratch {
    size_t bt, bgid, BK[2], BV[2], end;
    explicit BigScratch(uint32_t nbig)
    {
        rounds_detail::Carver carve(64);
        bt = carve((size_t)nbig * 4);
        bgid = carve((size_t)nbig * 4);
        BK[0] = carve((size_t)nbig * 8);
        BK[1] = carve((size_t)nbig * 8);
        BV[0] = carve((size_t)nbig * 4);
        BV[1] = carve((size_t)nbig * 4);
        end = carve.o;
    }
    static size_t reserved(uint32_t nbig) { return (size_t)nbig * (4 + 4 + 16 + 8) + 1024; }
};

// Slot S_PER: the periodic keys of a rank round (per_*_kernel).  The second (key, value) pair of its sort is BK[1] /
// BV[1] of BigScratch.  The five group arrays and the three result words lie in one region that is zeroed at once.
struct PerScratch {
    size_t g4;                  // bytes of one group array
    size_t PK0, PV0, step, flag, c, epos, eell, etail, pmin, zeroed, end;
    size_t zeroed_bytes;
    size_t gsize, links, bad, pg, out;
    PerScratch(uint32_t nbig, uint32_t nbig_groups)
    {
        using rounds_detail::up;
        g4 = up((size_t)nbig_groups * 4, 64);
        const size_t e4 = up((size_t)nbig * 4, 64), e8 = up((size_t)nbig * 8 + 8, 64);
        rounds_detail::Carver carve(1);      // (every size is rounded already)
        PK0 = carve(e8);
        PV0 = carve(e4);
        step = carve(e4);
        flag = carve(e4);
        c = carve(e8);
        epos = carve(e4);
        eell = carve(e4);
        etail = carve(e8);
        pmin = carve(g4);
        zeroed_bytes = 4 * g4 + 256;
        zeroed = carve(zeroed_bytes);
        gsize = zeroed;
        links = gsize + g4;
        bad = links + g4;
        pg = bad + g4;
        out = pg + g4;
        end = carve.o;
    }
    size_t reserved() const { return end; }
};

// Slot S_BGT: the segmented merge sort's group starts, the scan of their tile counts and the tiles.
struct BigTiles {
    uint32_t bound;             // tiles at most: one odd tile per group
    size_t gstart, toff, tiles, end;
    BigTiles(uint32_t nbig, uint32_t nbig_groups) : bound(nbig / BG_TILE + nbig_groups + 2)
    {
        rounds_detail::Carver carve(64);
        gstart = carve(((size_t)nbig_groups + 2) * 4);
        toff = carve(((size_t)nbig_groups + 2) * 8);
        tiles = carve((size_t)bound * sizeof(BigTile));
        end = carve.o;
    }
    size_t reserved() const { return end + 256; }
};

// Slot S_ANC + level: the selection pass of an anchor round over a string of n symbols.
struct AnchorScratch {
    uint32_t num_tiles;
    size_t m_cap;               // anchors the list Q holds (the round declines above n / cap_div)
    size_t dist_bytes;
    size_t dist, tile_cnt, tile_off, partial, Q, end;
    static constexpr size_t TOTAL_AT = ROUNDS_SCAN_BLOCKS;
    AnchorScratch(uint32_t n, uint32_t cap_div)
        : num_tiles((uint32_t)(((uint64_t)n + ANC_TILE - 1) / ANC_TILE)), m_cap((size_t)(n / cap_div) + 64),
          dist_bytes(rounds_detail::up((size_t)n, 16) + 16)
    {
        rounds_detail::Carver carve(64);
        dist = carve(dist_bytes);
        tile_cnt = carve((size_t)num_tiles * 4);
        tile_off = carve(((size_t)num_tiles + 2) * 8);
        partial = carve((ROUNDS_SCAN_BLOCKS + 8) * 8);
        Q = carve(m_cap * 4);
        end = carve.o;
    }
    size_t reserved() const
    {
        return dist_bytes + rounds_detail::up((size_t)num_tiles * 4, 64) + ((size_t)num_tiles + 2) * 8 + (ROUNDS_SCAN_BLOCKS + 8) * 8 +
               m_cap * 4 + 1024;
    }
};

// The anchors' own sort of m anchors, inside the caller's two key buffers of 8 n bytes each: the two key arrays in the
// first, nine index arrays in the second -- or, where level 0 has more anchors than that buffer holds nine arrays of, in
// a slot of their own (S_ANCW).  A string too small for either declines the round.
struct AnchorSort {
    enum Where { in_key_buffers, own_slot, decline };
    Where where;
    size_t m8, m4;
    size_t AK[2];               // in the first key buffer
    size_t AV[2], isa, AP[2], grp, grp2, sa, rank;      // in the second, or in the slot
    size_t second_bytes;        // what the nine arrays take
    AnchorSort(uint32_t n, uint32_t m, int level)
    {
        using rounds_detail::up;
        m8 = up((size_t)m * 8, 256);
        m4 = up((size_t)m * 4 + 64, 256);
        second_bytes = 9 * m4;
        const size_t buf = (size_t)n * 8;
        if (2 * m8 > buf) where = decline;              // (tiny strings)
        else if (second_bytes <= buf) where = in_key_buffers;
        else where = level == 0 ? own_slot : decline;
        AK[0] = 0;
        AK[1] = m8;
        AV[0] = 0;
        AV[1] = m4;
        isa = 2 * m4;
        AP[0] = 3 * m4;
        AP[1] = 4 * m4;
        grp = 5 * m4;
        grp2 = 6 * m4;
        sa = 7 * m4;
        rank = 8 * m4;
    }
};

// ---- the rules -----------------------------------------------------------------------------------------------------

// Bits of a rank 0 .. n | of an index or a group number 0 .. n - 1.
inline int rank_bits(uint32_t n)
{
    int bits = 1;
    while ((1ull << bits) <= (uint64_t)n) ++bits;
    return bits;
}
inline int index_bits(uint32_t n)
{
    int bits = 1;
    while ((1ull << bits) < (uint64_t)n) ++bits;
    return bits;
}
// Symbols of b bits each a 64-bit text-round key holds.
inline int symbols_per_key(int b) { return 64 / b > 16 ? 16 : 64 / b; }

enum RoundMode { M_DENSE = 0, M_SPARSE = 1, M_TEXT = 2 };

// Round 0: few ties: sparse (hash + key search); otherwise extend the ties from the text first.  m_next: the suffixes
// the initial sort left tied; knob_mode: PSS_MODE (-1 = choose).
inline RoundMode first_mode(uint32_t n, uint32_t m_next, uint64_t h, int knob_mode, int text_rounds_max, bool rank_only, bool subset,
                            bool no_sparse, uint64_t stop_text_h)
{
    RoundMode mode = ((uint64_t)m_next * 1024 <= (uint64_t)n) ? M_SPARSE : M_TEXT;
    if (knob_mode >= 0) mode = (RoundMode)knob_mode;
    if (mode == M_SPARSE && (uint64_t)m_next * 16 > (uint64_t)n) mode = M_TEXT;   // hash table must fit the ISA buffer
    if (mode == M_SPARSE && no_sparse && m_next) mode = M_TEXT;
    if (m_next == 0) mode = M_SPARSE;                                            // nothing left: no ISA at all
    if (mode == M_TEXT && text_rounds_max <= 0) mode = M_DENSE;
    if (rank_only && m_next) mode = M_DENSE;                                     // no text to pack keys from
    if (subset && m_next) mode = h < stop_text_h ? M_TEXT : M_DENSE;
    return mode;
}

// A text round gives up (nothing of it is kept) when more than half of its list sits in large groups -- in the first
// round only when it is more than three quarters.  Subset sorts run their text rounds whatever they resolve.
inline bool text_round_gives_up(uint32_t nbig, uint32_t m, int text_rounds, bool subset)
{
    return !subset && (uint64_t)nbig * 2 > (uint64_t)m && (text_rounds > 0 || (uint64_t)nbig * 4 > (uint64_t)m * 3);
}

// The large groups: the segmented merge sort or two chained radix sorts.  Default (round 6): the merge sort where the
// large groups are small on average (<= 2^16 members: `words`, source-like text -- a handful of tile sorts and merge
// passes inside every group against 8 + 3 chained radix passes over all of them), the chained sorts where a few groups
// hold millions (`mixed`: twelve merge passes against seven).  Measured: words 35.5-36.0 -> 35.2-35.4 ms, `source`
// 3-6 ms on one box and within the noise on another, mixed / dup_blocks / real files unchanged (forced on everywhere:
// mixed 88 -> 91).
enum BigRoute { BIG_CHAIN = 0, BIG_MERGE = 1 };
inline BigRoute big_route(int big_merge_knob, uint32_t nbig, uint32_t nbig_groups, bool use_text, int key_bits)
{
    const bool merge_auto = big_merge_knob < 0 && (uint64_t)nbig <= ((uint64_t)nbig_groups << 16);
    const bool merge = big_merge_knob == 1 || merge_auto || (big_merge_knob == 2 && use_text && key_bits > 32);
    return merge && nbig < 0x7fffffffu ? BIG_MERGE : BIG_CHAIN;
}

// The probe (probe_repeats_kernel): `same` of `pairs` sampled tied pairs share 48 more symbols.  No text round at all |
// the anchors sorted beside the text round.
inline bool probe_skips_text(bool deep_enough, uint32_t pairs, uint32_t same, int skip_pct)
{
    return deep_enough && pairs >= 64 && (uint64_t)same * 100 > (uint64_t)pairs * (uint64_t)skip_pct;
}
inline bool probe_wants_side(bool side_on, bool skip_text, uint32_t pairs, uint32_t same, int side_pct)
{
    return side_on && !skip_text && pairs >= 64 && (uint64_t)same * 100 >= (uint64_t)pairs * (uint64_t)side_pct;
}

// The three words the periodic-key pass reads back: members of periodic groups, members with equal steps, the smallest
// step.  Most of the list in chains whose step the depth has not reached: nothing to find before it has (the depth to
// wait for, 0: none) | the round met periodic runs, or chains that will be.
inline uint64_t per_wait(uint32_t per_members, uint32_t arith, uint32_t min_step, uint32_t nbig)
{
    return (per_members == 0 && (uint64_t)arith * 2 >= (uint64_t)nbig && min_step != 0xffffffffu) ? min_step : 0;
}
inline bool per_seen(uint32_t per_members, uint32_t arith, uint32_t nbig) { return per_members != 0 || (uint64_t)arith * 4 >= (uint64_t)nbig; }

// Rank rounds are group-local unless large groups dominate (repetitive data) -- then one global radix sort on (group
// rank, rank) with constant digits skipped is cheaper than ranking in LDS + compaction + two chained sorts over nearly
// everything.  The list length above which the rounds stay global (0: they stay local).  (periodic runs: the local
// rounds know a shortcut)
inline uint32_t goes_global(double last_big_frac, bool last_per, uint32_t m) { return last_big_frac > 0.5 && !last_per ? m / 2 : 0; }

// The 8-bit digits of a global round's key that vary, from the or / and of all keys.
inline uint32_t varying_digits(uint64_t vor, uint64_t vand, int key_bits)
{
    const uint64_t varying = vor & ~vand;
    uint32_t mask = 0;
    for (int p = 0; p < (key_bits + 7) / 8; ++p)
        if ((varying >> (8 * p)) & 0xffull) mask |= 1u << p;
    return mask;
}

}  // namespace pss
