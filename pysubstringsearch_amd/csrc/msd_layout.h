// msd_layout.h -- what the host drivers and the kernels of msd_sort.hip / ss_sort_impl.h have to agree on: the geometry
// of the two partition passes and the tile plan, the rows of their tables, the geometry of the sample sort, and the ONE
// description of the workspace both sorts carve their tables from (MsdWork).  Plain C++ without HIP, like build_plan.h:
// everything here is arithmetic on n (tests/native/msd_layout.cpp restates it on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

namespace pss {

// ---- geometry of the hybrid MSD sort (msd_sort.hip) ----------------------------------------------------------------

constexpr int MSD_D = 10;
constexpr uint32_t MSD_BINS = 1u << MSD_D;
constexpr int MSD_BLOCK = 512;
constexpr int MSD_IPT = 16;
constexpr uint32_t MSD_TILE = MSD_BLOCK * MSD_IPT;        // 8192 elements
constexpr uint32_t MSD_TILE2 = 16384;                     // elements of a tile of the wide scatter kernels and the look-back pass
constexpr uint32_t MSD_WIN = 6144;                        // buckets whose start falls into one window of this size share a tile ...
constexpr uint32_t MSD_TILE_CAP = 8176;                   // ... unless that is more than a tile holds: then the window's last bucket goes alone
                                                          // (the eight slots behind a tile's last element hold the sentinels of the fast
                                                          //  kernel's ranking window -- at most eight wide --, the eight after those its scalars)
constexpr uint32_t MSD_MAX_BUCKET = 4088;                 // a bucket must fit a tile on its own (the last eight slots of the LDS tile
                                                          // carry the fast kernel's scalars: MSD_TILE_CAP)
constexpr int MSD_TAG_BITS = MSD_D + 1;                   // an element entering the local sort carries the low 11 bits of its joint bucket number ...
constexpr uint32_t MSD_TAG_SPAN = 1u << MSD_TAG_BITS;     // ... so a tile never crosses a multiple of 2048 buckets: inside it the tags only grow
constexpr int MSD_RAW_TAG_BITS = 6;                       // LSD order: the tag is the joint bucket number mod 64 (= d mod 64) ...
constexpr uint32_t MSD_RAW_TAG_SPAN = 1u << MSD_RAW_TAG_BITS;   // ... and a tile stays inside one aligned block of 64 joint buckets
constexpr uint32_t MSD_G1_RANGES = 1024;
constexpr uint32_t MSD_G2_RANGE = 16 * MSD_TILE;          // elements per G2 range (a piece of one G1 bucket)
constexpr uint32_t MSD_SCAN_BLOCKS = 1024;                // SC_MAX_BLOCKS of scan.h (which needs HIP): partial sums of a device_excl_scan

struct MsdRange {
    uint32_t seg, start, end;
};

// A tile of the local sort
struct MsdTile {
    uint32_t e0, count, tag0, nb;      // first element, elements, tag of the first bucket, buckets
};

// A tile of the look-back pass: a piece of one d-region (count 0: an empty region, which still owes its row of the
// joint table), the region's digit, bit 31 = the region's last tile
struct MsdTile2 {
    uint32_t start, count, d_last;
};

// ---- geometry of the sample sort (ss_sort_impl.h) ------------------------------------------------------------------

constexpr int SS_MAX_CHARS = 32;                          // symbols packed into a key at most (byte window of the packers)
// Tile plan (msd_tile_head): the buckets that start inside one window of SS_WIN slots form a tile -- W elements on
// average, give or take what the buckets at its two ends overhang -- unless that exceeds the tile, in which case the
// window's last bucket becomes a tile of its own.  The merge sort costs per tile, not per element, so the window is as
// wide as the overflows allow: at 2^29 (buckets of 512 +- 256) 3072 -> 175 995 tiles, 3456 -> 161 659 (local sort 11.0 ->
// 10.0 ms), 3584 -> 160 905 but more of them single buckets (10.2 ms).
#ifndef PSS_SS_WIN
#define PSS_SS_WIN 3456
#endif
constexpr uint32_t SS_WIN = PSS_SS_WIN;

inline int msd_index_bits(uint32_t n)
{
    int ib = 1;
    while ((1ull << ib) < (uint64_t)n) ++ib;
    return ib;
}

struct SsGeometry {
    uint32_t B1, B2, os, S;
    int ib, kc, key_bits;
    uint64_t plo, phi;          // radix^(kc - 1)
};
inline bool ss_geometry(uint32_t n, uint32_t radix, SsGeometry *g)
{
    if (n < (1u << 16) || n > (1u << 30) || radix < 2 || radix > 257) return false;
    const int ib = msd_index_bits(n);
    // symbols per key: the largest kc with radix^kc <= 2^(128 - ib), at most SS_MAX_CHARS
    const unsigned __int128 limit = (unsigned __int128)1 << (128 - ib);
    unsigned __int128 pw = 1;
    int kc = 0;
    while (kc < SS_MAX_CHARS && pw <= limit / radix) {
        pw *= radix;
        ++kc;
    }
    if (kc < 2) return false;
    unsigned __int128 lead = 1;
    for (int i = 0; i + 1 < kc; ++i) lead *= radix;
    g->plo = (uint64_t)lead;
    g->phi = (uint64_t)(lead >> 64);
    int kb = 0;
    while (kb < 128 && ((pw - 1) >> kb) != 0) ++kb;      // bits of the largest key
    g->key_bits = kb;
    // joint buckets of ~512 elements (a tile holds 4088): B1 x B2 of them, both powers of two <= 1024
    int lb = 4;
    while (((uint64_t)512 << lb) < (uint64_t)n && lb < 20) ++lb;
    const uint32_t B1 = 1u << ((lb + 1) / 2), B2 = 1u << (lb / 2);
    // sample members per bucket: the bucket sizes follow a gamma distribution of that shape -- 4 puts a bucket of 512 on
    // average beyond 4088 with probability 1e-10, an average of 1024 (n = 2^30) needs 8
    const uint32_t os = ((uint64_t)n > (uint64_t)768 * B1 * B2) ? 8u : 4u;
    g->B1 = B1;
    g->B2 = B2;
    g->os = os;
    g->S = os * B1 * B2;
    g->ib = ib;
    g->kc = kc;
    return (uint64_t)g->S * 4 <= (uint64_t)n;
}
// Everything about the sort that depends on n and the alphabet, in one number (ss_geometry_tag of msd_sort.h)
inline uint64_t ss_geometry_pack(const SsGeometry &g)
{
    return ((uint64_t)g.S << 32) | ((uint64_t)g.B1 << 20) | ((uint64_t)g.B2 << 8) | ((uint64_t)g.ib << 2) | (uint64_t)(g.os == 8) | ((uint64_t)g.kc << 58);
}

// ---- table sizes ---------------------------------------------------------------------------------------------------

// Upper bound on the tiles of the plan: at most two per MSD_WIN window (msd_tile_head) plus one per aligned block
// of MSD_TAG_SPAN non-empty / MSD_RAW_TAG_SPAN joint buckets.
inline size_t msd_max_tiles(uint32_t n)
{
    return (size_t)n / (SS_WIN / 2) + ((size_t)MSD_BINS * MSD_BINS) / MSD_RAW_TAG_SPAN + 8;  // (the smaller window of the two paths, the
                                                                                             //  finer block rule: LSD order)
}
inline size_t msd_max_tiles2(uint32_t n) { return (size_t)n / MSD_TILE2 + MSD_BINS + 8; }

// Largest key width (bits of packed key >> drop) the 8-byte elements can carry for n suffixes, in LSD or MSD order:
// [bucket tag | K - 20 key bits | ib index bits] must fit 64 bits after the second pass (an 11-bit tag, or 6 bits in LSD
// order), and [K - 10 key bits | ib index bits] after the first
inline int msd_max_key_bits(uint32_t n, bool lsd)
{
    const int ib = msd_index_bits(n);
    const int after2 = 64 + MSD_D - (lsd ? MSD_RAW_TAG_BITS : MSD_TAG_BITS) - ib + MSD_D;
    const int after1 = 64 + MSD_D - ib;
    return after2 < after1 ? after2 : after1;
}

// ---- the workspace -------------------------------------------------------------------------------------------------

// Every table of the two sorts, in the order it lies in `work`; every region starts on a multiple of 256 bytes.  The
// sample sort uses the first thirteen (up to `shared_end`), the MSD sort in LSD order all eighteen; the size of the
// workspace is the end of all eighteen whatever the order (msd_workspace_bytes does not depend on a switch).
constexpr size_t MSD_TILE_PAD = 16;      // slots behind the max_tiles rows of the two tile tables
struct MsdWork {
    uint32_t *T = nullptr;              // [max_ranges2][1024] counts, then global offsets
    uint32_t *J1 = nullptr;             // [1025] bucket starts of the first pass
    uint32_t *J = nullptr;              // [2^20 + 1] joint bucket starts
    MsdRange *ranges2 = nullptr;        // [max_ranges2] ranges of the second pass
    uint32_t *seg_first = nullptr;      // [1025] first range of every first-pass bucket (before that: scratch of the offsets kernels)
    uint32_t *counters = nullptr;       // 16 words: [0] ranges, [1] largest joint bucket, [2] non-empty buckets, [3] tiles,
                                        // [4] tiles the fast local sort declined, [5] active records
    uint64_t *ranks = nullptr;          // [2^20 + 1] output of the scans
    uint32_t *cstart = nullptr;         // [2^20] starts of the non-empty joint buckets
    MsdTile *tiles_all = nullptr;       // [max_tiles] the plan
    uint32_t *tile_first = nullptr;     // [tile_first_slots()] first bucket of every tile and a sentinel; behind them the fail list
    uint32_t *blk_cnt = nullptr;        // [max_tiles] active records per tile
    uint64_t *dst_off = nullptr;        // [max_tiles + 1] where every tile's records go
    uint64_t *partial = nullptr;        // [MSD_SCAN_BLOCKS] partial sums of the scans; behind them the scans' totals
    // LSD order
    uint32_t *T2 = nullptr;             // [1024][MSD_G1_RANGES] counts of the first digit per range (only their totals are used)
    uint32_t *Jb = nullptr;             // [1025] starts of the first digit's buckets
    MsdTile2 *tiles2 = nullptr;         // [max_tiles2] tiles of the look-back pass
    uint32_t *status = nullptr;         // [max_tiles2][1024] look-back words
    uint32_t *cj = nullptr;             // [2^20] joint bucket number of every non-empty bucket

    size_t max_ranges2 = 0, max_tiles = 0, max_tiles2 = 0;
    size_t status_bytes = 0;            // (zeroed before every look-back pass)
    size_t shared_end = 0, end = 0;     // offsets behind the thirteenth and the last region

    // Lays the regions out from `base` (which may be null: the members are then the offsets) and returns the end offset.
    size_t lay(void *base, uint32_t n)
    {
        const uintptr_t b = reinterpret_cast<uintptr_t>(base);
        size_t o = 0;
        auto carve = [&](auto *&p, size_t bytes) {
            p = reinterpret_cast<decltype(+p)>(b + o);
            o = (o + bytes + 255) / 256 * 256;
        };
        const size_t nbk = (size_t)MSD_BINS * MSD_BINS;
        max_ranges2 = (size_t)n / MSD_G2_RANGE + MSD_BINS + 8;
        max_tiles = msd_max_tiles(n);
        max_tiles2 = msd_max_tiles2(n);
        status_bytes = max_tiles2 * MSD_BINS * 4;
        carve(T, max_ranges2 * MSD_BINS * 4);
        carve(J1, (MSD_BINS + 8) * 4);
        carve(J, (nbk + 8) * 4);
        carve(ranges2, max_ranges2 * sizeof(MsdRange));
        carve(seg_first, (MSD_BINS + 8) * 4);
        carve(counters, 64);
        carve(ranks, (nbk + 8) * 8);
        carve(cstart, (nbk + 8) * 4);
        carve(tiles_all, (max_tiles + MSD_TILE_PAD) * sizeof(MsdTile));
        carve(tile_first, tile_first_slots() * 4);
        carve(blk_cnt, (max_tiles + 8) * 4);
        carve(dst_off, (max_tiles + 8) * 8);
        carve(partial, PARTIAL_SLOTS * 8);
        shared_end = o;
        carve(T2, (size_t)MSD_BINS * MSD_G1_RANGES * 4);
        carve(Jb, (MSD_BINS + 8) * 4);
        carve(tiles2, max_tiles2 * sizeof(MsdTile2));
        carve(status, status_bytes);
        carve(cj, (nbk + 8) * 4);
        return end = o;
    }
    // MSD order: the kernels tell the order by these being null (msd_tile_head, msd_compact_kernel, msd_tile_desc_kernel)
    void drop_lsd_regions()
    {
        T2 = Jb = status = cj = nullptr;
        tiles2 = nullptr;
    }

    // Two arrays live inside another's region.
    // 1. The fail list -- numbers of the tiles the fast local sort declined, at most nt of them -- lies behind the tile
    //    firsts (nt + 1 of them with their sentinel): where the plan is made on the device, before the host knows nt, at
    //    max_tiles + MSD_TILE_PAD; where the host knows nt, at nt + 8.  Both fit for every nt <= max_tiles, which the
    //    drivers check before anything reads the list.
    size_t tile_first_slots() const { return 2 * (max_tiles + MSD_TILE_PAD); }
    size_t fail_list_at_planned_on_device() const { return max_tiles + MSD_TILE_PAD; }
    static size_t fail_list_at(uint32_t nt) { return (size_t)nt + 8; }
    bool fail_list_fits(size_t at, uint32_t nt) const { return at > (size_t)nt && at + nt <= tile_first_slots(); }
    // 2. The totals of two scans lie behind the partial sums.
    static constexpr size_t PARTIAL_SLOTS = MSD_SCAN_BLOCKS + 8;
    static constexpr size_t TOTAL_AT = MSD_SCAN_BLOCKS, TOTAL2_AT = MSD_SCAN_BLOCKS + 1;
    uint64_t *d_total() const { return partial + TOTAL_AT; }
    uint64_t *d_total2() const { return partial + TOTAL2_AT; }
};
static_assert(MsdWork::TOTAL_AT >= MSD_SCAN_BLOCKS && MsdWork::TOTAL2_AT > MsdWork::TOTAL_AT &&
                  MsdWork::TOTAL2_AT < MsdWork::PARTIAL_SLOTS,
              "the scans' totals lie behind the partial sums, inside their region");
static_assert(2 * MSD_TILE_PAD >= 8, "the fail list at nt + 8, nt <= max_tiles entries long, ends inside the 2 (max_tiles + pad) slots of tile_first");

// Bytes of workspace the sorts need besides their element buffers: the end of the layout.
inline size_t msd_workspace_bytes(uint32_t n) { return MsdWork().lay(nullptr, n); }

}  // namespace pss
