// The workspace layout and the geometry of the two initial sorts (csrc/msd_layout.h) checked on the CPU.
//
// model() below is the layout RESTATED: the eighteen region sizes in order, written out in plain numbers from the carve
// the drivers had before the header existed -- it calls none of the header's size expressions.  Every region of MsdWork
// must start where the model's running, 256-rounded offset puts it, and msd_workspace_bytes must be the model's end.  A
// few ends are pinned as numbers.  Then the two places where one array lives inside another's region, the tile caps, the
// largest key width, and one line per (n, radix) of ss_geometry, which tests/test_host.py compares with the Python model
// of the sample sort (tests/ss_edge_texts.geometry).
// Exit code 0 and "msd_layout: ok" = every check holds.  Built by tests/test_host.py with g++ -fsanitize=address,undefined
// against msd_layout.h alone.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msd_layout.h"

using namespace pss;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

constexpr int REGIONS = 18, SHARED = 13;

struct Model {
    uint64_t size[REGIONS], start[REGIONS], shared_end, end;
    uint64_t max_tiles, max_tiles2;
};
static Model model(uint64_t n)
{
    Model m;
    const uint64_t ranges2 = n / 131072 + 1024 + 8;      // second-pass ranges of 16 x 8192 elements, one odd one per bucket
    const uint64_t nbk = 1048576;                        // joint buckets
    m.max_tiles = n / 1728 + 16384 + 8;                  // two per window of 3456, one per block of 64 joint buckets
    m.max_tiles2 = n / 16384 + 1024 + 8;
    const uint64_t sizes[REGIONS] = {
        ranges2 * 1024 * 4,            // T
        (1024 + 8) * 4,                // J1
        (nbk + 8) * 4,                 // J
        ranges2 * 12,                  // ranges2
        (1024 + 8) * 4,                // seg_first
        64,                            // counters
        (nbk + 8) * 8,                 // ranks
        (nbk + 8) * 4,                 // cstart
        (m.max_tiles + 16) * 16,       // tiles_all
        (m.max_tiles + 16) * 8,        // tile_first (and the fail list)
        (m.max_tiles + 8) * 4,         // blk_cnt
        (m.max_tiles + 8) * 8,         // dst_off
        (1024 + 8) * 8,                // partial (and the totals)
        1024ull * 1024 * 4,            // T2
        (1024 + 8) * 4,                // Jb
        m.max_tiles2 * 12,             // tiles2
        m.max_tiles2 * 1024 * 4,       // status
        (nbk + 8) * 4,                 // cj
    };
    uint64_t o = 0;
    for (int r = 0; r < REGIONS; ++r) {
        m.size[r] = sizes[r];
        m.start[r] = o;
        o = (o + sizes[r] + 255) / 256 * 256;
        if (r == SHARED - 1) m.shared_end = o;
    }
    m.end = o;
    return m;
}

static void regions_of(const MsdWork &w, uintptr_t out[REGIONS])
{
    const void *p[REGIONS] = {w.T,         w.J1,         w.J,       w.ranges2, w.seg_first, w.counters, w.ranks,  w.cstart, w.tiles_all,
                              w.tile_first, w.blk_cnt,    w.dst_off, w.partial, w.T2,        w.Jb,       w.tiles2, w.status, w.cj};
    for (int r = 0; r < REGIONS; ++r) out[r] = reinterpret_cast<uintptr_t>(p[r]);
}

static void check_layout(uint32_t n)
{
    const Model m = model(n);
    const uintptr_t base = (uintptr_t)1 << 40;      // (never dereferenced)
    MsdWork w;
    const size_t end = w.lay(reinterpret_cast<void *>(base), n);
    uintptr_t at[REGIONS];
    regions_of(w, at);
    for (int r = 0; r < REGIONS; ++r) {
        CHECK(at[r] == base + m.start[r]);
        CHECK(at[r] % 256 == 0);
        if (r > 0) CHECK(at[r] >= at[r - 1] + m.size[r - 1]);      // ascending, no overlap
    }
    CHECK(end == m.end && w.end == m.end && end >= m.start[REGIONS - 1] + m.size[REGIONS - 1]);
    CHECK(w.shared_end == m.shared_end);
    CHECK(msd_workspace_bytes(n) == m.end);
    // a null base gives the offsets themselves
    MsdWork z;
    CHECK(z.lay(nullptr, n) == m.end);
    regions_of(z, at);
    for (int r = 0; r < REGIONS; ++r) CHECK(at[r] == m.start[r]);
    // MSD order: the five LSD regions are null, the thirteen shared ones stay
    z.drop_lsd_regions();
    regions_of(z, at);
    for (int r = 0; r < REGIONS; ++r) CHECK(at[r] == (r < SHARED ? m.start[r] : 0));
    // table capacities
    CHECK(w.max_tiles == m.max_tiles && msd_max_tiles(n) == m.max_tiles);
    CHECK(w.max_tiles2 == m.max_tiles2 && msd_max_tiles2(n) == m.max_tiles2);
    CHECK(w.status_bytes == m.size[16]);
    // the fail list behind the tile firsts: at both of its positions it holds nt = max_tiles entries behind the
    // nt + 1 tile firsts, inside the region
    const uint64_t slots = m.size[9] / 4, mt = m.max_tiles;
    CHECK(w.tile_first_slots() == slots && slots == 2 * (mt + 16));
    CHECK(w.fail_list_at_planned_on_device() == mt + 16);
    CHECK(mt + 16 + mt <= slots && mt + 16 > mt);
    CHECK(MsdWork::fail_list_at((uint32_t)mt) == mt + 8 && mt + 8 + mt <= slots);
    for (uint64_t nt : {(uint64_t)0, (uint64_t)1, mt / 2, mt}) {
        CHECK(w.fail_list_fits(w.fail_list_at_planned_on_device(), (uint32_t)nt));
        CHECK(w.fail_list_fits(MsdWork::fail_list_at((uint32_t)nt), (uint32_t)nt));
    }
    CHECK(!w.fail_list_fits(MsdWork::fail_list_at((uint32_t)mt + 13), (uint32_t)mt + 13));      // (2 mt + 34 slots)
    // the two totals behind the partial sums
    CHECK(MsdWork::TOTAL_AT == 1024 && MsdWork::TOTAL2_AT == 1025);
    CHECK((MsdWork::TOTAL2_AT + 1) * 8 <= m.size[12]);
}

static void check_pointers_in_real_memory()
{
    const uint32_t n = 2;
    std::vector<unsigned char> mem(msd_workspace_bytes(n));
    MsdWork w;
    w.lay(mem.data(), n);
    CHECK(w.d_total() == w.partial + 1024 && w.d_total2() == w.partial + 1025);
    CHECK(reinterpret_cast<unsigned char *>(w.d_total2() + 1) <= reinterpret_cast<unsigned char *>(w.T2));
    *w.d_total() = 1;      // (inside the allocation: the sanitizer looks on)
    *w.d_total2() = 2;
    w.cj[1048576 - 1] = 3;
    w.tile_first[w.fail_list_at_planned_on_device() + w.max_tiles - 1] = 4;
    CHECK(reinterpret_cast<unsigned char *>(w.cj + 1048576) <= mem.data() + mem.size());
}

static void check_pinned()
{
    const struct { uint32_t n; uint64_t end; } ends[] = {
        {65536u, 34276352ull}, {1u << 24, 39340800ull}, {1u << 29, 196880896ull}, {0x7fffffffu, 684739072ull}};
    for (const auto &e : ends) CHECK(msd_workspace_bytes(e.n) == e.end);
    const struct { uint32_t n; uint64_t shared_end, tiles, tiles2; } rows[] = {
        {65536u, 21627136ull, 16429, 1036}, {1u << 24, 22501376ull, 26101, 2056}, {1u << 29, 49637120ull, 327081, 33800}};
    for (const auto &r : rows) {
        MsdWork w;
        w.lay(nullptr, r.n);
        CHECK(w.shared_end == r.shared_end);
        CHECK(msd_max_tiles(r.n) == r.tiles && msd_max_tiles2(r.n) == r.tiles2);
    }
}

static void check_key_bits()
{
    for (uint32_t n : {2u, 1u << 20, 1u << 29, 1u << 30}) {
        int ib = 1;
        while ((1ull << ib) < n) ++ib;
        CHECK(msd_index_bits(n) == ib);
        for (int lsd = 0; lsd < 2; ++lsd) {
            // [tag | K - 2 D key bits | ib] and [K - D key bits | ib] fit 64 bits
            const int tag = lsd ? MSD_RAW_TAG_BITS : MSD_TAG_BITS;
            const int after2 = 64 - tag - ib + 2 * MSD_D, after1 = 64 - ib + MSD_D;
            const int want = after2 < after1 ? after2 : after1;
            CHECK(msd_max_key_bits(n, lsd != 0) == want);
            CHECK(tag + (want - 2 * MSD_D) + ib <= 64 && (want - MSD_D) + ib <= 64);
        }
    }
    CHECK(msd_max_key_bits(1u << 29, true) == 45 && msd_max_key_bits(1u << 29, false) == 44);
}

static void print_geometry()
{
    int tags = 0;
    for (uint32_t n : {65535u, 65536u, 1u << 20, 1u << 24, 1u << 30, (1u << 30) + 1}) {
        for (uint32_t radix : {1u, 2u, 28u, 257u, 258u}) {
            SsGeometry g;
            if (!ss_geometry(n, radix, &g)) {
                printf("geometry %u %u refused\n", n, radix);
                continue;
            }
            printf("geometry %u %u %d %d %d %u %u %u %u\n", n, radix, g.ib, g.kc, g.key_bits, g.B1, g.B2, g.os, g.S);
            // radix^(kc - 1), the two halves
            unsigned __int128 lead = 1;
            for (int i = 0; i + 1 < g.kc; ++i) lead *= radix;
            CHECK(g.plo == (uint64_t)lead && g.phi == (uint64_t)(lead >> 64));
            if ((radix == 28 || radix == 257) && (n == (1u << 24) || n == (1u << 30)) && tags < 4) {
                printf("tag %u %u %" PRIu64 "\n", n, radix, ss_geometry_pack(g));
                ++tags;
            }
        }
    }
}

int main()
{
    for (uint32_t n : {2u, 3u, 15634u, 65535u, 65536u, 1u << 20, 1u << 24, (1u << 24) + 1, 1u << 29, (1u << 30) - 1, 1u << 30, 0x7fffffffu})
        check_layout(n);
    check_pointers_in_real_memory();
    check_pinned();
    check_key_bits();
    print_geometry();
    printf("msd_layout: ok\n");
    return 0;
}
