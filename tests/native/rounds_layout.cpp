// The scratch layouts and the decision rules of the rounds (csrc/rounds_layout.h) checked on the CPU.
//
// Every layout is RESTATED below as a table of region sizes in order, written out in plain numbers from the carve
// sequences the driver had before the header existed -- the tables call none of the header's size expressions.  Every
// region must start where the table's running, rounded offset puts it, `end` must be the table's end, and the end must
// lie inside what the slot reserved before the header existed (the old formulas, written out here as well).  Then the
// three outcomes of AnchorSort on both sides of their boundaries, and every rule walked over its edges with the
// expected answers written down, not recomputed.
// Exit code 0 and "rounds_layout: ok" = every check holds.  Built by tests/test_host.py with g++
// -fsanitize=address,undefined against rounds_layout.h alone.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rounds_layout.h"

using namespace pss;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const char *g_what = "";
static uint64_t g_a = 0, g_b = 0;
// (a failing layout check says which layout at which sizes)
#define CHECK_AT(cond)                                                                                                  \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            fprintf(stderr, "%s:%d: %s  [%s %" PRIu64 " %" PRIu64 "]\n", __FILE__, __LINE__, #cond, g_what, g_a, g_b);    \
            exit(1);                                                                                                    \
        }                                                                                                               \
    } while (0)

static uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

static const uint64_t SIZES[] = {1, 2, 255, 256, 257, 512, 513, 2047, 2048, 2049, 4096, 4097, 1ull << 20, (1ull << 24) + 1, (1ull << 31) - 1, (1ull << 32) - 1};

// starts of regions of the given sizes, each start on a multiple of `align`; returns the end
static uint64_t lay(const std::vector<uint64_t> &sizes, uint64_t align, std::vector<uint64_t> *starts)
{
    uint64_t o = 0;
    starts->clear();
    for (uint64_t sz : sizes) {
        starts->push_back(o);
        o = up(o + sz, align);
    }
    return o;
}
static void check_regions(const std::vector<uint64_t> &sizes, uint64_t align, const std::vector<size_t> &got, size_t got_end, uint64_t old_reservation)
{
    std::vector<uint64_t> want;
    const uint64_t end = lay(sizes, align, &want);
    CHECK_AT(got.size() == want.size());
    for (size_t r = 0; r < got.size(); ++r) {
        CHECK_AT(got[r] == want[r]);
        CHECK_AT(got[r] % 64 == 0);
        if (r > 0) CHECK_AT(got[r] >= got[r - 1] + sizes[r - 1]);      // ascending, no overlap
    }
    CHECK_AT(got_end == end);
    CHECK_AT(got_end >= want.back() + sizes.back());
    CHECK_AT(got_end <= old_reservation);
}

static void check_round_scratch(uint64_t m, bool mid_tier)
{
    g_what = mid_tier ? "RoundScratch+mid" : "RoundScratch";
    g_a = m;
    g_b = 0;
    const uint64_t nblk = (m + 2047) / 2048;
    std::vector<uint64_t> sizes = {m, nblk * 4, nblk * 4, (nblk + 1) * 8, (nblk + 1) * 8, (1024 + 2) * 8};
    if (mid_tier) {
        sizes.push_back((m / 2 + 16) * 8);
        sizes.push_back((m / 512 + 16) * 8);
        sizes.push_back(64);
    }
    const uint64_t old_reservation = m + nblk * 24 + (1024 + 8) * 8 + 4096 + (m / 2 + 16) * 8 + (m / 512 + 16) * 8 + 512;
    const RoundScratch L((uint32_t)m, mid_tier);
    std::vector<size_t> got = {L.big, L.blk_big, L.blk_heads, L.off_big, L.off_heads, L.partial};
    if (mid_tier) {
        got.push_back(L.mid);
        got.push_back(L.mid_fail);
        got.push_back(L.mid_count);
    }
    check_regions(sizes, 64, got, L.end, old_reservation);
    CHECK_AT(L.nblk == nblk);
    CHECK_AT(RoundScratch::reserved((uint32_t)m) == old_reservation);      // the slot asks for what it asked for
    CHECK_AT(RoundScratch::TOTAL_AT == 1024 && (RoundScratch::TOTAL_AT + 1) * 8 <= sizes[5]);
}

static void check_big_scratch(uint64_t nbig)
{
    g_what = "BigScratch";
    g_a = nbig;
    g_b = 0;
    const std::vector<uint64_t> sizes = {nbig * 4, nbig * 4, nbig * 8, nbig * 8, nbig * 4, nbig * 4};
    const uint64_t old_reservation = nbig * (4 + 4 + 16 + 8) + 1024;
    const BigScratch B((uint32_t)nbig);
    check_regions(sizes, 64, {B.bt, B.bgid, B.BK[0], B.BK[1], B.BV[0], B.BV[1]}, B.end, old_reservation);
    CHECK_AT(BigScratch::reserved((uint32_t)nbig) == old_reservation);
}

static void check_per_scratch(uint64_t nbig, uint64_t groups)
{
    g_what = "PerScratch";
    g_a = nbig;
    g_b = groups;
    const uint64_t g4 = up(groups * 4, 64), e4 = up(nbig * 4, 64), e8 = up(nbig * 8 + 8, 64);
    // (every size is a multiple of 64 already: the regions follow each other without rounding)
    const std::vector<uint64_t> sizes = {e8, e4, e4, e4, e8, e4, e4, e8, g4, 4 * g4 + 256};
    const uint64_t old_reservation = e8 + e4 + e4 + e4 + e8 + e4 + e4 + e8 + 5 * g4 + 256;
    const PerScratch Y((uint32_t)nbig, (uint32_t)groups);
    check_regions(sizes, 1, {Y.PK0, Y.PV0, Y.step, Y.flag, Y.c, Y.epos, Y.eell, Y.etail, Y.pmin, Y.zeroed}, Y.end, old_reservation);
    CHECK_AT(Y.end == old_reservation && Y.reserved() == old_reservation);      // exactly the carve sequence
    CHECK_AT(Y.g4 == g4 && Y.zeroed_bytes == 4 * g4 + 256);
    // the five arrays zeroed together: four group arrays, then the result words
    CHECK_AT(Y.gsize == Y.zeroed && Y.links == Y.zeroed + g4 && Y.bad == Y.zeroed + 2 * g4 && Y.pg == Y.zeroed + 3 * g4 && Y.out == Y.zeroed + 4 * g4);
    CHECK_AT(Y.out + 3 * 4 <= Y.zeroed + Y.zeroed_bytes && Y.zeroed + Y.zeroed_bytes == Y.end);
    CHECK_AT(groups * 4 <= g4 && nbig * 4 <= e4 && (nbig + 1) * 8 <= e8);
}

static void check_big_tiles(uint64_t nbig, uint64_t groups)
{
    g_what = "BigTiles";
    g_a = nbig;
    g_b = groups;
    const uint64_t bound = nbig / 4096 + groups + 2;
    const std::vector<uint64_t> sizes = {(groups + 2) * 4, (groups + 2) * 8, bound * 12};
    const uint64_t old_reservation = up((groups + 2) * 4, 64) + up((groups + 2) * 8, 64) + up(bound * 12, 64) + 256;
    const BigTiles T((uint32_t)nbig, (uint32_t)groups);
    check_regions(sizes, 64, {T.gstart, T.toff, T.tiles}, T.end, old_reservation);
    CHECK_AT(T.bound == bound);
    CHECK_AT(T.end + 256 == old_reservation && T.reserved() == old_reservation);
    // a tile per 4096 members of every group, one odd one per group at most
    CHECK_AT(bound >= (nbig + 4095) / 4096 + groups - (groups ? 1 : 0));
}

static void check_anchor_scratch(uint64_t n, uint64_t cap_div)
{
    g_what = "AnchorScratch";
    g_a = n;
    g_b = cap_div;
    const uint64_t tiles = (n + 4095) / 4096, n16 = up(n, 16) + 16, m_cap = n / cap_div + 64;
    const std::vector<uint64_t> sizes = {n16, tiles * 4, (tiles + 2) * 8, (1024 + 8) * 8, m_cap * 4};
    const uint64_t old_reservation = n16 + up(tiles * 4, 64) + (tiles + 2) * 8 + (1024 + 8) * 8 + m_cap * 4 + 1024;
    const AnchorScratch A((uint32_t)n, (uint32_t)cap_div);
    check_regions(sizes, 64, {A.dist, A.tile_cnt, A.tile_off, A.partial, A.Q}, A.end, old_reservation);
    CHECK_AT(A.num_tiles == tiles && A.m_cap == m_cap && A.dist_bytes == n16);
    CHECK_AT(A.reserved() == old_reservation);
    CHECK_AT(AnchorScratch::TOTAL_AT == 1024 && (AnchorScratch::TOTAL_AT + 1) * 8 <= sizes[3]);
    CHECK_AT(n / cap_div <= m_cap);      // a round that does not decline lists at most n / cap_div anchors
}

static void check_layouts()
{
    for (uint64_t x : SIZES) {
        check_round_scratch(x, false);
        check_round_scratch(x, true);
        check_big_scratch(x);
        for (uint64_t cap_div : {3, 4, 5}) check_anchor_scratch(x, cap_div);
        for (uint64_t g : {(uint64_t)1, (uint64_t)2, x / 2}) {
            if (g == 0 || g > x / 2) continue;      // (a large group has two members at least)
            check_per_scratch(x, g);
            check_big_tiles(x, g);
        }
    }
}

// Real memory of exactly the reserved size, the last byte of every region written: the sanitizer looks on.
static void check_in_real_memory()
{
    {
        const uint32_t m = 4097;
        std::vector<unsigned char> mem(RoundScratch::reserved(m));
        const RoundScratch L(m, true);
        mem[L.big + m - 1] = 1;
        mem[L.off_heads + ((size_t)L.nblk + 1) * 8 - 1] = 1;
        mem[L.partial + (RoundScratch::TOTAL_AT + 1) * 8 - 1] = 1;
        mem[L.mid + ((size_t)m / 2 + 16) * 8 - 1] = 1;
        mem[L.mid_fail + ((size_t)m / 512 + 16) * 8 - 1] = 1;
        mem[L.mid_count + 7] = 1;
        CHECK(L.end <= mem.size());
    }
    {
        const uint32_t nbig = 513, groups = 7;
        const PerScratch Y(nbig, groups);
        std::vector<unsigned char> mem(Y.reserved());
        mem[Y.etail + ((size_t)nbig + 1) * 8 - 1] = 1;
        mem[Y.out + 11] = 1;
        const BigTiles T(nbig, groups);
        std::vector<unsigned char> tm(T.reserved());
        tm[T.tiles + (size_t)T.bound * sizeof(BigTile) - 1] = 1;
        const BigScratch B(nbig);
        std::vector<unsigned char> bm(BigScratch::reserved(nbig));
        bm[B.BV[1] + (size_t)nbig * 4 - 1] = 1;
        const AnchorScratch A(nbig, 5);
        std::vector<unsigned char> am(A.reserved());
        am[A.Q + A.m_cap * 4 - 1] = 1;
    }
}

// The rule as the driver had it, in its two places.
static AnchorSort::Where old_anchor_rule(uint64_t n, uint64_t m, int level)
{
    const uint64_t m8 = up(m * 8, 256), m4 = up(m * 4 + 64, 256);
    bool own = false;
    if (level == 0 && 9 * m4 > n * 8 && 2 * m8 <= n * 8) own = true;
    if (2 * m8 > n * 8 || (!own && 9 * m4 > n * 8)) return AnchorSort::decline;
    return own ? AnchorSort::own_slot : AnchorSort::in_key_buffers;
}
static void check_anchor_sort()
{
    // 9 * m4 against 8 n: n = 28800 (8 n = 230400 = 9 * 25600), m = 6384 gives m4 = 25600
    CHECK(AnchorSort(28800, 6384, 0).where == AnchorSort::in_key_buffers);
    CHECK(AnchorSort(28800, 6384, 1).where == AnchorSort::in_key_buffers);
    CHECK(AnchorSort(28800, 6385, 0).where == AnchorSort::own_slot);       // m4 = 25856: a slot of their own on level 0 ...
    CHECK(AnchorSort(28800, 6385, 1).where == AnchorSort::decline);        // ... and no round a level up
    CHECK(AnchorSort(28800, 6385, 0).second_bytes == 9 * 25856);
    // 2 * m8 against 8 n: n = 640 (8 n = 5120), m = 320 gives m8 = 2560
    CHECK(AnchorSort(640, 320, 0).where == AnchorSort::own_slot);          // (nine arrays of 1536 bytes do not fit 5120)
    CHECK(AnchorSort(640, 320, 1).where == AnchorSort::decline);
    CHECK(AnchorSort(640, 321, 0).where == AnchorSort::decline);           // m8 = 2816: tiny string
    CHECK(AnchorSort(640, 321, 1).where == AnchorSort::decline);
    // the eleven arrays, where they lie
    const AnchorSort A(1u << 20, 1000, 0);
    CHECK(A.where == AnchorSort::in_key_buffers && A.m8 == 8192 && A.m4 == 4096);
    CHECK(A.AK[0] == 0 && A.AK[1] == 8192);
    const size_t second[9] = {A.AV[0], A.AV[1], A.isa, A.AP[0], A.AP[1], A.grp, A.grp2, A.sa, A.rank};
    for (size_t k = 0; k < 9; ++k) CHECK(second[k] == k * 4096);
    CHECK(A.second_bytes == 9 * 4096);
    // every (n, m, level) of a sweep against the old two-place rule; what is not declined fits where it is put
    for (uint64_t n : {64ull, 65ull, 288ull, 640ull, 1000ull, 4096ull, 28800ull})
        for (uint64_t m = 1; m <= n; ++m)
            for (int level = 0; level < 3; ++level) {
                const AnchorSort S((uint32_t)n, (uint32_t)m, level);
                CHECK(S.where == old_anchor_rule(n, m, level));
                if (S.where != AnchorSort::decline) CHECK(S.AK[1] + m * 8 <= n * 8);
                if (S.where == AnchorSort::in_key_buffers) CHECK(S.rank + m * 4 <= n * 8);
                if (S.where == AnchorSort::own_slot) CHECK(S.rank + m * 4 <= S.second_bytes && level == 0);
            }
    for (uint64_t n : SIZES)
        for (uint64_t m : {(uint64_t)1, n / 5, n / 3, n})
            for (int level = 0; level < 2; ++level)
                if (m) CHECK(AnchorSort((uint32_t)n, (uint32_t)m, level).where == old_anchor_rule(n, m, level));
}

static void check_bits()
{
    CHECK(rank_bits(1) == 1 && rank_bits(2) == 2 && rank_bits(3) == 2 && rank_bits(4) == 3);
    CHECK(index_bits(1) == 1 && index_bits(2) == 1 && index_bits(3) == 2 && index_bits(4) == 2 && index_bits(5) == 3);
    for (int k = 2; k < 32; ++k) {
        const uint32_t p = 1u << k;
        CHECK(rank_bits(p - 1) == k && rank_bits(p) == k + 1 && rank_bits(p + 1) == k + 1);      // ranks 0 .. n
        CHECK(index_bits(p - 1) == k && index_bits(p) == k && index_bits(p + 1) == k + 1);       // indices 0 .. n - 1
    }
    CHECK(rank_bits(0xffffffffu) == 32 && index_bits(0xffffffffu) == 32 && rank_bits(0x80000000u) == 32 && index_bits(0x80000000u) == 31);
    const int want[10] = {0, 16, 16, 16, 16, 12, 10, 9, 8, 7};
    for (int b = 1; b <= 9; ++b) CHECK(symbols_per_key(b) == want[b]);
}

static void check_first_mode()
{
    const uint32_t n = 1u << 20;
    // (n, m_next, h, knob, text_rounds_max, rank_only, subset, no_sparse, stop_text_h)
    CHECK(first_mode(n, 1023, 8, -1, 5, false, false, false, 0) == M_SPARSE);
    CHECK(first_mode(n, 1024, 8, -1, 5, false, false, false, 0) == M_SPARSE);      // m_next * 1024 == n
    CHECK(first_mode(n, 1025, 8, -1, 5, false, false, false, 0) == M_TEXT);
    // sparse forced: the hash table must fit the ISA buffer
    CHECK(first_mode(n, 65535, 8, 1, 5, false, false, false, 0) == M_SPARSE);
    CHECK(first_mode(n, 65536, 8, 1, 5, false, false, false, 0) == M_SPARSE);      // m_next * 16 == n
    CHECK(first_mode(n, 65537, 8, 1, 5, false, false, false, 0) == M_TEXT);
    // nothing left tied: sparse, whatever else is said
    for (int knob = -1; knob <= 2; ++knob)
        for (int flags = 0; flags < 8; ++flags)
            CHECK(first_mode(n, 0, 8, knob, flags & 1 ? 0 : 5, (flags & 2) != 0, (flags & 4) != 0, true, 20) == M_SPARSE);
    // each forced mode
    CHECK(first_mode(n, 1, 8, 0, 5, false, false, false, 0) == M_DENSE);
    CHECK(first_mode(n, 1, 8, 1, 5, false, false, false, 0) == M_SPARSE);
    CHECK(first_mode(n, 1, 8, 2, 5, false, false, false, 0) == M_TEXT);
    CHECK(first_mode(n, 1, 8, 2, 0, false, false, false, 0) == M_DENSE);           // no text rounds allowed
    CHECK(first_mode(n, 2000, 8, -1, 0, false, false, false, 0) == M_DENSE);
    CHECK(first_mode(n, 2000, 8, -1, -1, false, false, false, 0) == M_DENSE);
    // the sample sort's key does not fit the key search
    CHECK(first_mode(n, 1, 8, -1, 5, false, false, true, 0) == M_TEXT);
    CHECK(first_mode(n, 1, 8, 1, 5, false, false, true, 0) == M_TEXT);
    CHECK(first_mode(n, 1, 8, 0, 5, false, false, true, 0) == M_DENSE);
    // integer strings: rank rounds, whatever the knob says
    for (int knob = -1; knob <= 2; ++knob) {
        CHECK(first_mode(n, 1, 1, knob, 5, true, false, false, 0) == M_DENSE);
        CHECK(first_mode(n, n, 1, knob, 5, true, false, false, 0) == M_DENSE);
    }
    // subset sorts: text rounds up to the depth asked for, then rank rounds
    for (int knob = -1; knob <= 2; ++knob) {
        CHECK(first_mode(n, 1, 8, knob, 5, false, true, true, 9) == M_TEXT);
        CHECK(first_mode(n, 1, 8, knob, 0, false, true, true, 9) == M_TEXT);
        CHECK(first_mode(n, 1, 8, knob, 5, false, true, true, 8) == M_DENSE);
        CHECK(first_mode(n, 1, 9, knob, 5, false, true, true, 8) == M_DENSE);
    }
    // no overflow at the top
    CHECK(first_mode(0xffffffffu, 0xffffffffu, 8, -1, 5, false, false, false, 0) == M_TEXT);
    CHECK(first_mode(0xffffffffu, 0xffffffffu, 8, 1, 5, false, false, false, 0) == M_TEXT);
    CHECK(first_mode(0xffffffffu, 4194303u, 8, -1, 5, false, false, false, 0) == M_SPARSE);      // 4194303 * 1024 = 2^32 - 1024
    CHECK(first_mode(0xffffffffu, 4194304u, 8, -1, 5, false, false, false, 0) == M_TEXT);
}

static void check_gives_up()
{
    // (nbig, m, text_rounds, subset)
    for (int tr = 0; tr < 2; ++tr) {
        CHECK(!text_round_gives_up(499, 1000, tr, false));
        CHECK(!text_round_gives_up(500, 1000, tr, false));      // 2 nbig == m
    }
    CHECK(!text_round_gives_up(501, 1000, 0, false));
    CHECK(text_round_gives_up(501, 1000, 1, false));
    CHECK(!text_round_gives_up(749, 1000, 0, false));
    CHECK(!text_round_gives_up(750, 1000, 0, false));           // 4 nbig == 3 m
    CHECK(text_round_gives_up(751, 1000, 0, false));
    CHECK(text_round_gives_up(749, 1000, 1, false) && text_round_gives_up(750, 1000, 1, false) && text_round_gives_up(751, 1000, 1, false));
    for (int tr = 0; tr < 2; ++tr)
        for (uint32_t nbig : {501u, 751u, 1000u}) CHECK(!text_round_gives_up(nbig, 1000, tr, true));
    CHECK(text_round_gives_up(0xffffffffu, 0xffffffffu, 0, false));      // (64-bit products)
    CHECK(!text_round_gives_up(0x7fffffffu, 0xffffffffu, 1, false));
    CHECK(text_round_gives_up(0x80000000u, 0xffffffffu, 1, false));
}

static void check_big_route()
{
    // (knob, nbig, nbig_groups, use_text, key_bits): three groups, 3 << 16 = 196608 members
    CHECK(big_route(-1, 196607, 3, false, 21) == BIG_MERGE);
    CHECK(big_route(-1, 196608, 3, false, 21) == BIG_MERGE);      // nbig == nbig_groups << 16
    CHECK(big_route(-1, 196609, 3, false, 21) == BIG_CHAIN);
    CHECK(big_route(-1, 65536, 1, true, 64) == BIG_MERGE && big_route(-1, 65537, 1, true, 64) == BIG_CHAIN);
    for (uint32_t nbig : {196607u, 196608u, 196609u, 0x7ffffffeu, 0x7fffffffu, 0xffffffffu}) {
        CHECK(big_route(0, nbig, 3, true, 64) == BIG_CHAIN);
        CHECK(big_route(1, nbig, 3, false, 21) == (nbig < 0x7fffffffu ? BIG_MERGE : BIG_CHAIN));
        CHECK(big_route(2, nbig, 3, false, 64) == BIG_CHAIN);       // in text rounds only
        CHECK(big_route(2, nbig, 3, true, 32) == BIG_CHAIN);        // ... whose keys are wider than 32 bits
        CHECK(big_route(2, nbig, 3, true, 33) == (nbig < 0x7fffffffu ? BIG_MERGE : BIG_CHAIN));
    }
    // the tile table counts in 32 bits: never the merge sort from 2^31 - 1 members on
    CHECK(big_route(-1, 0x7ffffffeu, 0x8000, false, 21) == BIG_MERGE);
    CHECK(big_route(-1, 0x7fffffffu, 0x8000, false, 21) == BIG_CHAIN);
    CHECK(big_route(-1, 0xffffffffu, 0x7fffffffu, false, 21) == BIG_CHAIN);
    CHECK(big_route(-1, 0x7ffffffeu, 0x7fff, false, 21) == BIG_CHAIN);      // 0x7fff << 16 = 2^31 - 65536
}

static void check_probe()
{
    // (deep_enough, pairs, same, skip_pct)
    CHECK(!probe_skips_text(true, 63, 63, 50));
    CHECK(!probe_skips_text(true, 64, 32, 50));      // exactly the percentage: not more than
    CHECK(probe_skips_text(true, 64, 33, 50));
    CHECK(!probe_skips_text(false, 64, 64, 50));
    CHECK(probe_skips_text(true, 8192, 4097, 50) && !probe_skips_text(true, 8192, 4096, 50));
    CHECK(probe_skips_text(true, 100, 1, 0) && !probe_skips_text(true, 100, 100, 100));
    // (side_on, skip_text, pairs, same, side_pct)
    CHECK(!probe_wants_side(true, false, 63, 63, 8));
    CHECK(probe_wants_side(true, false, 64, 6, 8) && !probe_wants_side(true, false, 64, 5, 8));      // 600 >= 512 > 500
    CHECK(probe_wants_side(true, false, 100, 8, 8) && !probe_wants_side(true, false, 100, 7, 8));    // exactly the percentage: at least
    CHECK(!probe_wants_side(false, false, 100, 100, 8));
    CHECK(!probe_wants_side(true, true, 100, 100, 8));
}

static void check_periodic_and_global()
{
    // (per_members, arith, min_step, nbig)
    CHECK(per_wait(0, 5, 77, 10) == 77);                 // half of the list in chains
    CHECK(per_wait(0, 4, 77, 10) == 0);
    CHECK(per_wait(1, 5, 77, 10) == 0);                  // something was found: nothing to wait for
    CHECK(per_wait(0, 5, 0xffffffffu, 10) == 0);         // no step recorded
    CHECK(per_wait(0, 0x80000000u, 0xfffffffeu, 0xffffffffu) == 0xfffffffeull);
    CHECK(per_seen(1, 0, 12) && per_seen(0, 3, 12) && !per_seen(0, 2, 12) && !per_seen(0, 0, 1));
    // (last_big_frac, last_per, m)
    CHECK(goes_global(0.5, false, 100) == 0);
    CHECK(goes_global(0.51, false, 100) == 50 && goes_global(1.0, false, 101) == 50);
    CHECK(goes_global(0.51, true, 100) == 0 && goes_global(1.0, true, 100) == 0);
    // (or, and, key_bits)
    CHECK(varying_digits(0xff00, 0, 16) == 2u && varying_digits(0xff00, 0, 8) == 0u);
    CHECK(varying_digits(0x1234, 0x1234, 64) == 0u);
    CHECK(varying_digits(0x100000001ull, 0, 33) == 0x11u && varying_digits(0x100000001ull, 0, 32) == 0x1u);
    CHECK(varying_digits(0x100000001ull, 1, 40) == 0x10u);
    CHECK(varying_digits(~0ull, 0, 64) == 0xffu && varying_digits(~0ull, 0, 57) == 0xffu && varying_digits(~0ull, 0, 56) == 0x7fu);
}

int main()
{
    CHECK(GS_T == 2048 && GS_CAP == 512 && MID_CAP == 4096 && MID_KMAX == 512 && BG_TILE == 4096 && ANC_TILE == 4096 && ROUNDS_SCAN_BLOCKS == 1024);
    CHECK(sizeof(MidGroup) == 8 && sizeof(BigTile) == 12);
    check_layouts();
    check_in_real_memory();
    check_anchor_sort();
    check_bits();
    check_first_mode();
    check_gives_up();
    check_big_route();
    check_probe();
    check_periodic_and_global();
    printf("rounds_layout: ok\n");
    return 0;
}
