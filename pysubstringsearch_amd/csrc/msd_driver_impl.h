// msd_driver_impl.h -- the host side of the two initial sorts: msd_suffix_sort (msd_sort.hip) and ss_suffix_sort
// (ss_sort_impl.h) as staged drivers.  Included at the end of msd_sort.hip, inside namespace pss, behind every kernel.
//
// A driver is a small object: the arguments, the route (every switch read ONCE, in the constructor), the tables of the
// workspace (MsdWork, msd_layout.h: the one place that says where they lie) and one member function per stage.  run()
// is the list of stages; a stage that ends in a host wait says so in its name's comment.  DESIGN.md 4.2 / 4.3.

static_assert(MSD_SCAN_BLOCKS == SC_MAX_BLOCKS, "msd_layout.h restates the partial sums of scan.h");
static_assert(MSD_G1_RANGES <= 1024, "msd_offsets1_kernel takes four ranges per thread");
static_assert(SS_SBLOCK == (int)MSD_BINS, "one bin per thread in the scatter passes");

// LSD order + look-back: the default wherever its 30-bit look-back words hold the positions.  PSS_MSD_LSD=0: the two
// passes in MSD order with the second histogram pass (rounds 2-5).
static bool msd_use_lsd(uint32_t n)
{
    const char *e = knob("PSS_MSD_LSD");
    return !(e && atoi(e) == 0) && n < (1u << 30);
}

int msd_max_key_bits(uint32_t n) { return msd_max_key_bits(n, msd_use_lsd(n)); }

// ---- what both drivers share -----------------------------------------------------------------------------------------

// The pinned words a sort reads back (h_small: the head of the caller's pinned block -- SmallState of sa_refine_impl.h
// views the same memory as plain words, and reads none of them across a sort).
struct MsdReadback {
    u32 total, total_hi;       // [0] the 64-bit total the stage in flight asked for last: non-empty buckets; tiles of a plan made
                               //     with the host; (one word) tiles the fast kernel declined on that route; entries of the
                               //     gathered active list, and in the high word the suffixes msd_finish_kernel settled
    u32 counters[4];           // [2] counters 0 .. 3 of the workspace: ranges, largest joint bucket, non-empty buckets, tiles
    u32 bad_symbol;            // [6] MsdFront: a byte of the text had no code
    u32 unused7;
    u32 tiles_dev, tiles_dev_hi;   // [8] tiles of a plan made on the device (the total of its scan)
    u32 declined_dev;          // [10] ... and the tiles the fast kernel declined of them
};
static_assert(offsetof(MsdReadback, counters) == 8 && offsetof(MsdReadback, bad_symbol) == 24 && offsetof(MsdReadback, tiles_dev) == 32 &&
                  offsetof(MsdReadback, declined_dev) == 40 && sizeof(MsdReadback) <= 64,
              "h_small is 64 bytes, and the words lie where they always lay");

// Profile mode: named begin / end events on the stream, one event where a stage ends and the next begins.  Off: no
// event call at all.
enum Stage { ST_SAMPLE, ST_G1, ST_G2, ST_LOCAL, ST_COUNT };
struct StageTimes {
    hipStream_t s;
    bool on;
    hipEvent_t ev[2 * ST_COUNT] = {};
    int nev = 0;
    int at[ST_COUNT][2];
    StageTimes(hipStream_t s_, bool on_) : s(s_), on(on_)
    {
        for (auto &p : at) p[0] = p[1] = -1;
    }
    StageTimes(const StageTimes &) = delete;
    StageTimes &operator=(const StageTimes &) = delete;
    ~StageTimes()
    {
        for (int i = 0; i < nev; ++i) (void)hipEventDestroy(ev[i]);
    }
    int mark(Stage ends, Stage begins)      // (ST_COUNT: none)
    {
        if (!on || nev >= 2 * ST_COUNT) return PSS_OK;
        PSS_HIP(hipEventCreate(&ev[nev]));
        const int e = nev++;
        PSS_HIP(hipEventRecord(ev[e], s));
        if (ends != ST_COUNT) at[ends][1] = e;
        if (begins != ST_COUNT) at[begins][0] = e;
        return PSS_OK;
    }
    int begin(Stage st) { return mark(ST_COUNT, st); }
    int end(Stage st) { return mark(st, ST_COUNT); }
    // (after a wait for the stream) out may be null
    int ms(Stage st, double *out) const
    {
        if (at[st][0] < 0 || at[st][1] < 0) return PSS_OK;
        float t = 0.f;
        PSS_HIP(hipEventElapsedTime(&t, ev[at[st][0]], ev[at[st][1]]));
        if (out) *out = t;
        return PSS_OK;
    }
};

// Both sorts partition twice into 2^20 joint buckets and plan tiles over the non-empty ones: the same thirteen tables
// and the same helper launches on them.
struct SortTables {
    DeviceCtx *ctx;
    hipStream_t s;
    u32 n;
    MsdWork w;
    MsdReadback *h;
    StageTimes times;
    u32 ne = 0, max_bucket = 0, nt = 0;      // non-empty buckets, the largest of them, tiles: known to the host after a wait
    static constexpr size_t nbk = (size_t)MSD_BINS * MSD_BINS;

    SortTables(DeviceCtx *c, u32 n_, void *work, u32 *h_small, bool profile)
        : ctx(c), s(c->stream), n(n_), h(reinterpret_cast<MsdReadback *>(h_small)), times(c->stream, profile)
    {
        w.lay(work, n);
    }
    // digit-major counts of a first pass -> offsets in place, and the 1025 bucket starts (w.seg_first: scratch for the totals)
    void first_offsets(u32 *counts, u32 num_ranges1, u32 *starts)
    {
        hipLaunchKernelGGL(msd_offsets1_kernel, dim3(MSD_BINS), dim3(256), 0, s, counts, num_ranges1, w.seg_first);
        hipLaunchKernelGGL(msd_offsets1b_kernel, dim3(1), dim3(MSD_BINS), 0, s, (const u32 *)w.seg_first, starts, n);
    }
    // the ranges of a second pass that stays inside the first pass's buckets; once they are counted, the joint table
    void second_ranges() { hipLaunchKernelGGL(msd_ranges_kernel, dim3(1), dim3(MSD_BINS), 0, s, (const u32 *)w.J1, w.ranges2, w.seg_first, w.counters); }
    void joint_offsets()
    {
        hipLaunchKernelGGL(msd_offsets_kernel, dim3(MSD_BINS), dim3(MSD_BINS), 0, s, w.T, (const u32 *)w.seg_first, (const u32 *)w.J1, w.J,
                           0u, n, MSD_BINS);
    }
    // non-empty joint buckets: their number (the scan's total), their starts, the largest (counters[1])
    int count_buckets(u32 *cj)
    {
        PSS_TRY(device_excl_scan(ctx, InNonEmpty{w.J}, nbk, w.partial, w.d_total(), w.ranks));
        hipLaunchKernelGGL(msd_compact_kernel, dim3(1024), dim3(256), 0, s, w.J, (u32)nbk, w.ranks, w.cstart, w.counters, cj);
        return PSS_OK;
    }
    int copy_bucket_counts()
    {
        PSS_HIP(hipMemcpyAsync(&h->total, w.d_total(), 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipMemcpyAsync(h->counters, w.counters, 16, hipMemcpyDeviceToHost, s));
        return PSS_OK;
    }
    void take_bucket_counts()      // (after the wait)
    {
        ne = h->total;
        max_bucket = h->counters[1];
    }
    // the window rule of msd_tile_head, the number of buckets known to the host
    int plan_windows(TilePlan tp)
    {
        PSS_TRY(device_excl_scan(ctx, InTileHead{w.cstart, ne, n, tp}, ne, w.partial, w.d_total(), w.ranks));
        hipLaunchKernelGGL(msd_tiles_kernel, dim3(1024), dim3(256), 0, s, w.cstart, ne, n, w.ranks, (const u64 *)w.d_total(), w.tile_first, tp);
        return PSS_OK;
    }
    // HOST WAIT: the number of tiles of the plan just launched (the total of its last scan)
    int wait_for_tiles(const char *who)
    {
        PSS_HIP(hipMemcpyAsync(&h->total, w.d_total(), 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        nt = h->total;
        return check_tiles(who);
    }
    // cannot happen (msd_max_tiles is an upper bound of the plan): never run past the tables.  With it the fail list fits
    // behind the tile firsts wherever it is put (MsdWork::fail_list_fits).
    int check_tiles(const char *who) const
    {
        if ((size_t)nt <= w.max_tiles) return PSS_OK;
        set_error("%s: %u tiles planned, tables hold %zu (internal error)", who, nt, w.max_tiles);
        return PSS_EDEVICE;
    }
    void describe_tiles(const u32 *cj)
    {
        hipLaunchKernelGGL(msd_tile_desc_kernel, dim3((nt + 255) / 256), dim3(256), 0, s, w.cstart, w.tile_first, nt, ne, n, w.tiles_all,
                           cj, (const u64 *)nullptr, (const u64 *)nullptr);
    }
};

// ---- hybrid MSD sort -------------------------------------------------------------------------------------------------

struct MsdSort : SortTables {
    const TextKeys *text;
    u64 *const *A;
    u32 *sa_out;
    MsdStats *stats;
    MsdActive *active;
    const MsdFront *front;
    // the route
    const bool lsd;             // digits in LSD order, second pass by look-back (else MSD order with a second histogram pass)
    const bool wide;            // 16384-element scatter tiles (MSD order with PSS_MSD_SCATTER=1: the 8192-element kernels)
    const bool slow_local;      // PSS_MSD_SLOW_LOCAL: every tile to the general local sort
    const bool one_trip;        // plan and local sort launched without the host: one wait tells it everything
    const bool fused;           // the local sort emits the active list of the first rerank
    const bool finish;          // ... and small tie groups are settled before the gather
    const int ib, rem_bits;
    MsdArgs a;
    MsdEmit em{};
    u32 *fail_list = nullptr;

    MsdSort(DeviceCtx *c, const TextKeys *text_, u32 n_, int key_bits, u64 *const *A_, u32 *sa_out_, void *work, u32 *h_small, bool profile,
            MsdStats *stats_, MsdActive *active_, const MsdFront *front_, bool lsd_)
        : SortTables(c, n_, work, h_small, profile), text(text_), A(A_), sa_out(sa_out_), stats(stats_), active(active_), front(front_),
          lsd(lsd_), wide(lsd_ || !(knob("PSS_MSD_SCATTER") && atoi(knob("PSS_MSD_SCATTER")) == 1)),
          slow_local(knob("PSS_MSD_SLOW_LOCAL") != nullptr), one_trip(lsd_ && !slow_local), fused(active_ != nullptr),
          finish(knob("PSS_MSD_NO_FINISH") == nullptr), ib(msd_index_bits(n_)), rem_bits(key_bits - 2 * MSD_D)
    {
        if (!lsd) w.drop_lsd_regions();
        if (fused) em = MsdEmit{active->st_pos, active->st_idx, w.blk_cnt};
        memset(&a, 0, sizeof a);
        a.codes = text->codes;
        a.code_bits = text->code_bits;
        a.key_chars = text->key_chars;
        a.plus_one = text->plus_one;
        a.key_drop = text->drop;
        a.n = n;
        a.key_bits = key_bits;
        a.idx_bits = ib;
        const u32 num_tiles = (u32)(((u64)n + MSD_TILE - 1) / MSD_TILE);
        a.tiles_per_range1 = (num_tiles + MSD_G1_RANGES - 1) / MSD_G1_RANGES;
        a.num_ranges1 = (num_tiles + a.tiles_per_range1 - 1) / a.tiles_per_range1;
        a.T = w.T;
        a.J1 = w.J1;
        a.J = w.J;
        a.ranges2 = w.ranges2;
        a.seg_first = w.seg_first;
        a.counters = w.counters;
        a.lsd = lsd ? 1 : 0;
        a.T2 = w.T2;
        a.Jb = w.Jb;
        a.tiles2 = w.tiles2;
        a.status = w.status;
    }

    // One pass over the text: the counts of the first pass's digit per range (LSD order: of both digits), and from them
    // where every (range, digit) goes.  With a `front` the pass reads the raw text and leaves the codes.
    int histograms()
    {
        PSS_HIP(hipMemsetAsync(w.counters, 0, 64, s));
        a.out = A[0];
        if (front) {
            a.raw = front->raw;
            a.lut = front->lut;
            a.codes_out = const_cast<u8 *>(text->codes);
            a.bad = front->bad;
            hipLaunchKernelGGL(msd_hist_raw_kernel, dim3(a.num_ranges1), dim3(MSD_BLOCK), 0, s, a);
        } else {
            hipLaunchKernelGGL(msd_hist_kernel<true>, dim3(a.num_ranges1), dim3(MSD_BLOCK), 0, s, a);
        }
        first_offsets(w.T, a.num_ranges1, w.J1);
        if (lsd) {
            // the first digit's bucket starts from the same pass over the text (the per-range prefixes in T2 are not used)
            first_offsets(w.T2, a.num_ranges1, w.Jb);
            // (the words of the look-back pass: zero = nothing published)
            PSS_HIP(hipMemsetAsync(w.status, 0, w.status_bytes, s));
        }
        return PSS_OK;
    }
    // text -> A[0].  16384-element scatter tiles (whole-line runs), 1024 threads: 2.2 -> 1.9 ms (from the text) and
    // 2.8 -> 2.45 ms (second pass, with its sixteen loads per thread issued before the ranking atomics) at 2^29; 512
    // threads x 32 elements spill.
    int first_pass()
    {
        PSS_TRY(times.begin(ST_G1));
        if (lsd) hipLaunchKernelGGL((msd_scatter2_kernel<true, 1024, true>), dim3(a.num_ranges1), dim3(1024), 0, s, a);
        else if (wide) hipLaunchKernelGGL((msd_scatter2_kernel<true, 1024>), dim3(a.num_ranges1), dim3(1024), 0, s, a);
        else hipLaunchKernelGGL(msd_scatter_kernel<true>, dim3(a.num_ranges1), dim3(MSD_BLOCK), 0, s, a);
        PSS_TRY(times.end(ST_G1));
        a.in = A[0];
        a.out = A[1];
        return PSS_OK;
    }
    // LSD order: A[0] -> A[1] by the first digit in one sweep, tile order kept (look-back); leaves the joint table
    int second_pass_lookback()
    {
        hipLaunchKernelGGL(msd_tiles2_kernel, dim3(1), dim3(MSD_BINS), 0, s, (const u32 *)w.J1, w.tiles2, w.counters);
        PSS_TRY(times.begin(ST_G2));
        const u32 grid2 = std::min<u32>((u32)w.max_tiles2, (u32)ctx->num_cus);      // one 1024-thread workgroup per CU (~100 VGPRs)
        hipLaunchKernelGGL(msd_scatter_lb_kernel, dim3(grid2), dim3(1024), 0, s, a);
        return times.end(ST_G2);
    }
    // MSD order: every first-pass bucket counted by the next 10 bits -> the joint table (the scatter waits for the verdict)
    int second_histogram()
    {
        second_ranges();
        a.dense = w.ranks;
        hipLaunchKernelGGL(msd_hist_kernel<false>, dim3((u32)w.max_ranges2), dim3(MSD_BLOCK), 0, s, a);
        joint_offsets();
        return PSS_OK;
    }
    // LSD order: nothing between the bucket counts and the local sort needs the host -- the counts stay on the device (the
    // scans run over all 2^20 bucket numbers), the local sort checks the plan's verdict itself, ONE round trip afterwards
    // tells the host everything (rounds 2-5: three, ~0.1 ms of idle GPU each at n = 2^29).
    int plan_and_sort_on_device()
    {
        u64 *const d_total = w.d_total(), *const d_total2 = w.d_total2();
        const TilePlan tp{MSD_WIN, MSD_TILE_CAP, w.cj};
        fail_list = w.tile_first + w.fail_list_at_planned_on_device();
        PSS_TRY(device_excl_scan(ctx, InTileHeadDev{w.cstart, d_total, n, tp}, nbk, w.partial, d_total2, w.ranks));
        hipLaunchKernelGGL(msd_tiles_dev_kernel, dim3(1024), dim3(256), 0, s, w.cstart, (const u64 *)d_total, n, w.ranks, (const u64 *)d_total2,
                           w.tile_first, tp);
        hipLaunchKernelGGL(msd_tile_desc_kernel, dim3((u32)((w.max_tiles + 255) / 256)), dim3(256), 0, s, w.cstart, w.tile_first, 0u, 0u, n,
                           w.tiles_all, (const u32 *)w.cj, (const u64 *)d_total2, (const u64 *)d_total);
        PSS_TRY(times.begin(ST_LOCAL));
        hipLaunchKernelGGL(msd_local_fast_kernel, dim3(2u * (u32)ctx->num_cus), dim3(MSD_BLOCK), 0, s, A[1], (const MsdTile *)w.tiles_all, 0u,
                           rem_bits, ib, sa_out, fail_list, w.counters + 4, (int)fused, em, (const u64 *)d_total2, (const u32 *)w.counters,
                           front ? (const u32 *)front->bad : (const u32 *)nullptr);
        PSS_TRY(times.end(ST_LOCAL));
        PSS_HIP(hipMemcpyAsync(&h->tiles_dev, d_total2, 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipMemcpyAsync(&h->declined_dev, w.counters + 4, 4, hipMemcpyDeviceToHost, s));
        return PSS_OK;
    }
    // HOST WAIT (the only one of the one-trip route before the gather's): buckets, the largest, the front's verdict.
    // *go = false: a byte the table has no code for (nothing of this sort can be used), or not this text (a bucket
    // beyond a tile: the caller takes the LSD path)
    int wait_for_counts(bool *go)
    {
        PSS_TRY(copy_bucket_counts());
        if (front) PSS_HIP(hipMemcpyAsync(&h->bad_symbol, front->bad, 4, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        take_bucket_counts();
        const u32 bad = front ? h->bad_symbol : 0u;
        if (stats) {
            stats->buckets = ne;
            stats->max_bucket = max_bucket;
            stats->bad_symbol = bad;
        }
        *go = !bad && max_bucket <= MSD_MAX_BUCKET;
        return PSS_OK;
    }
    // MSD order: A[0] -> A[1], every first-pass bucket by the next 10 bits
    int second_scatter()
    {
        PSS_TRY(times.begin(ST_G2));
        if (wide) hipLaunchKernelGGL((msd_scatter2_kernel<false, 1024>), dim3((u32)w.max_ranges2), dim3(1024), 0, s, a);
        else hipLaunchKernelGGL(msd_scatter_kernel<false>, dim3((u32)w.max_ranges2), dim3(MSD_BLOCK), 0, s, a);
        return times.end(ST_G2);
    }
    void general_local_sort(u32 tiles, const u32 *list)
    {
        hipLaunchKernelGGL(msd_local_sort_kernel, dim3(tiles), dim3(MSD_BLOCK), 0, s, A[1], (const MsdTile *)w.tiles_all, rem_bits, ib,
                           sa_out, list, (int)fused, em);
    }
    // one-trip route, after its wait: the tiles the fast kernel declined go to the general one
    int sort_declined_on_device_plan()
    {
        nt = h->tiles_dev;
        PSS_TRY(check_tiles("msd_suffix_sort"));
        const u32 nfail = h->declined_dev;
        if (stats) stats->slow_tiles = nfail;
        if (nfail) general_local_sort(nfail, fail_list);
        return PSS_OK;
    }
    // HOST WAIT: the plan with the number of buckets known to the host; the wait brings the number of tiles
    int plan_on_host()
    {
        PSS_TRY(plan_windows(TilePlan{MSD_WIN, MSD_TILE_CAP, w.cj}));
        PSS_TRY(wait_for_tiles("msd_suffix_sort"));
        PSS_TRY(times.begin(ST_LOCAL));
        // counters[4] = tiles the fast kernel declined (their numbers go behind the tile table), [5] = active records
        fail_list = w.tile_first + MsdWork::fail_list_at(nt);
        describe_tiles(w.cj);
        return PSS_OK;
    }
    int local_sort_slow()
    {
        general_local_sort(nt, nullptr);
        return times.end(ST_LOCAL);
    }
    // HOST WAIT: the fast kernel, then the tiles it declined
    int local_sort_fast()
    {
        const u32 grid = std::min<u32>(nt, 2u * (u32)ctx->num_cus);
        hipLaunchKernelGGL(msd_local_fast_kernel, dim3(grid), dim3(MSD_BLOCK), 0, s, A[1], (const MsdTile *)w.tiles_all, nt, rem_bits, ib,
                           sa_out, fail_list, w.counters + 4, (int)fused, em, (const u64 *)nullptr, (const u32 *)nullptr, (const u32 *)nullptr);
        PSS_TRY(times.end(ST_LOCAL));            // (profile mode) the events bracket this launch alone
        PSS_HIP(hipMemcpyAsync(&h->total, w.counters + 4, 4, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        const u32 nfail = h->total;
        if (stats) stats->slow_tiles = nfail;
        if (nfail) general_local_sort(nfail, fail_list);
        return PSS_OK;
    }
    // HOST WAIT.  Small groups are settled here and now (msd_finish_kernel); the list is made of what they leave.  The
    // count of the settled suffixes comes down with the list's length, in the high word of the same sum.
    int finish_and_gather()
    {
        if (finish) {
            const int ks = std::min(64 / text->code_bits, 16);
            const MsdFinish fin{text->codes, text->code_bits, ks, text->plus_one,
                                (u32)(text->drop ? text->key_chars - 1 : text->key_chars), n};
            hipLaunchKernelGGL(msd_finish_kernel, dim3((nt + 3) / 4), dim3(256), 0, s, (const MsdTile *)w.tiles_all, w.blk_cnt, nt,
                               active->st_pos, active->st_idx, sa_out, fin);
        }
        PSS_TRY(device_excl_scan(ctx, InBlkCnt{w.blk_cnt}, nt, w.partial, w.d_total(), w.dst_off));
        hipLaunchKernelGGL(msd_gather_kernel, dim3((nt + 3) / 4), dim3(256), 0, s, (const MsdTile *)w.tiles_all, w.blk_cnt, w.dst_off, nt,
                           active->st_pos, active->st_idx, active->pos, active->idx, active->grp);
        PSS_HIP(hipMemcpyAsync(&h->total, w.d_total(), 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        active->count = h->total;
        if (stats) stats->finished = h->total_hi;
        return PSS_OK;
    }
    int report()
    {
        if (stats) {
            stats->tiles = nt;
            stats->lookback = lsd ? 1u : 0u;
        }
        if (!times.on) return PSS_OK;
        PSS_HIP(hipStreamSynchronize(s));
        PSS_TRY(times.ms(ST_G1, stats ? &stats->ms_g1 : nullptr));
        PSS_TRY(times.ms(ST_G2, stats ? &stats->ms_g2 : nullptr));
        return times.ms(ST_LOCAL, stats ? &stats->ms_local : nullptr);
    }

    int run(bool *accepted)
    {
        PSS_TRY(histograms());
        PSS_TRY(first_pass());
        PSS_TRY(lsd ? second_pass_lookback() : second_histogram());
        PSS_TRY(count_buckets(w.cj));
        if (one_trip) PSS_TRY(plan_and_sort_on_device());
        bool go = false;
        PSS_TRY(wait_for_counts(&go));
        if (!go) return PSS_OK;
        if (!lsd) PSS_TRY(second_scatter());
        if (one_trip) {
            PSS_TRY(sort_declined_on_device_plan());
        } else {
            PSS_TRY(plan_on_host());
            PSS_TRY(slow_local ? local_sort_slow() : local_sort_fast());
        }
        if (fused) PSS_TRY(finish_and_gather());
        PSS_HIP(hipGetLastError());
        PSS_TRY(report());
        *accepted = true;
        return PSS_OK;
    }
};

int msd_suffix_sort(DeviceCtx *ctx, const TextKeys *text, uint32_t n, int key_bits, uint64_t *A[2], uint32_t *sa_out,
                    void *work, uint32_t *h_small, bool profile, MsdStats *stats, bool *accepted, MsdActive *active,
                    const MsdFront *front)
{
    *accepted = false;
    const bool lsd = msd_use_lsd(n);
    if (key_bits < 2 * MSD_D + 1 || key_bits > msd_max_key_bits(n, lsd) || n < 2) {
        set_error("msd_suffix_sort: key of %d bits does not fit (n = %u)", key_bits, n);
        return PSS_EINVAL;
    }
    MsdSort sort(ctx, text, n, key_bits, A, sa_out, work, h_small, profile, stats, active, front, lsd);
    return sort.run(accepted);
}

// ---- sample sort -------------------------------------------------------------------------------------------------------

uint32_t ss_sample_count(uint32_t n)
{
    SsGeometry g;
    return ss_geometry(n, 257, &g) ? g.S : 0u;
}
// Everything about the sort that depends on n and the alphabet, in one number (0: the sort does not take this text): two
// texts with the same tag can be cut by the same sorted sample (sa_build.hip, the plan of the sample sort).
uint64_t ss_geometry_tag(uint32_t n, uint32_t radix)
{
    SsGeometry g;
    return ss_geometry(n, radix, &g) ? ss_geometry_pack(g) : 0;
}
int ss_key_chars(uint32_t n, uint32_t radix)
{
    SsGeometry g;
    return ss_geometry(n, radix, &g) ? g.kc : 0;
}

struct SsSort : SortTables {
    const SsBuffers &buf;
    u32 *sa_out;
    SsStats *stats;
    const SsGeometry g;
    // the route: the local sort bucket by bucket over a padded greedy plan (default), the greedy plan unpadded
    // (PSS_SS_SEG=0), or the window plan of the MSD sort (PSS_SS_WINDOW_PLAN)
    const bool window_plan, seg, debug;
    const u32 S;
    const SsText tx;
    E16 *const E0;
    E16 *E;
    SsArgs a;
    u32 *pstart = nullptr;      // padded plan: the padded bucket starts (read by the local sort too)

    SsSort(DeviceCtx *c, const TextKeys *text, u32 radix, u32 n_, const SsGeometry &g_, const SsBuffers &buf_, u32 *sa_out_, void *work,
           u32 *h_small, bool profile, SsStats *stats_)
        : SortTables(c, n_, work, h_small, profile), buf(buf_), sa_out(sa_out_), stats(stats_), g(g_),
          window_plan(knob("PSS_SS_WINDOW_PLAN") != nullptr), seg(!window_plan && !(knob("PSS_SS_SEG") && atoi(knob("PSS_SS_SEG")) == 0)),
          debug(knob("PSS_SS_DEBUG") != nullptr), S(g_.S),
          tx{text->codes, n_, text->code_bits, g_.kc, text->plus_one, g_.ib, radix, g_.plo, g_.phi}, E0(static_cast<E16 *>(buf_.E0)),
          E(static_cast<E16 *>(buf_.E))
    {
        w.drop_lsd_regions();      // (the thirteen shared tables are all this sort uses)
        memset(&a, 0, sizeof a);
        a.text = tx;
        a.B1 = g.B1;
        a.B2 = g.B2;
        a.spb = S / g.B1;
        a.st2 = g.os;
        a.zl = (u32)std::max(0, std::min(64 - SS_CELL_BITS, 128 - g.key_bits - g.ib));
        const u32 num_tiles = (u32)(((u64)n + SS_DTILE1 - 1) / SS_DTILE1);
        a.tiles_per_range1 = (num_tiles + MSD_G1_RANGES - 1) / MSD_G1_RANGES;
        a.num_ranges1 = (num_tiles + a.tiles_per_range1 - 1) / a.tiles_per_range1;
        a.T = w.T;
        a.J1 = w.J1;
        a.ranges2 = w.ranges2;
        a.counters = w.counters;
        a.digits = buf.digits;
    }

    // The sample, sorted as 128-bit numbers (or the sorted sample the caller kept from the last chunk).
    // HOST WAITS (two) only where the sample is small enough to be sorted on the host.
    int sample()
    {
        if (buf.sample_in) {
            E = const_cast<E16 *>(static_cast<const E16 *>(buf.sample_in));      // (read only from here on)
            return PSS_OK;
        }
        hipLaunchKernelGGL(ss_sample_kernel, dim3((S + 255) / 256), dim3(256), 0, s, tx, S, E0, buf.K[0], buf.V[0]);
        if (S <= 8192) {
            // (small texts, tests: the device sort's one-workgroup path is not stable, which the second of the chained sorts needs)
            std::vector<E16> hs(S);
            PSS_HIP(hipMemcpyAsync(hs.data(), E0, (size_t)S * 16, hipMemcpyDeviceToHost, s));
            PSS_HIP(hipStreamSynchronize(s));
            std::sort(hs.begin(), hs.end(), [](const E16 &x, const E16 &y) { return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo); });
            PSS_HIP(hipMemcpyAsync(E, hs.data(), (size_t)S * 16, hipMemcpyHostToDevice, s));
            PSS_HIP(hipStreamSynchronize(s));
        } else {
            u64 *K[2] = {buf.K[0], buf.K[1]};
            u32 *V[2] = {buf.V[0], buf.V[1]};
            SortStats ss1;
            int d1 = 0, d2 = 0;
            PSS_TRY(radix_sort_pairs(ctx, K, V, S, 64, 0xffu, nullptr, 0, buf.sort_work, &d1, false, &ss1));
            hipLaunchKernelGGL(ss_gather_hi_kernel, dim3((S + 255) / 256), dim3(256), 0, s, E0, (const u32 *)V[d1], S, K[d1]);
            const int hi_bits = std::min(64, std::max(1, g.key_bits + g.ib - 64));
            PSS_TRY(radix_sort_pairs(ctx, K, V, S, hi_bits, 0xffu, nullptr, d1, buf.sort_work, &d2, false, &ss1));
            hipLaunchKernelGGL(ss_gather_elems_kernel, dim3((S + 255) / 256), dim3(256), 0, s, E0, (const u32 *)V[d2], S, E);
        }
        if (buf.sample_keep) PSS_HIP(hipMemcpyAsync(buf.sample_keep, E, (size_t)S * 16, hipMemcpyDeviceToDevice, s));
        return PSS_OK;
    }
    // text -> A[0] by the first-level splitters
    int first_pass()
    {
        a.sample = E;
        PSS_HIP(hipMemsetAsync(w.counters, 0, 64, s));
        hipLaunchKernelGGL(ss_digits1_kernel, dim3(a.num_ranges1), dim3(SS_DBLOCK), 0, s, a);
        first_offsets(w.T, a.num_ranges1, w.J1);
        a.out = static_cast<E16 *>(buf.A[0]);
        hipLaunchKernelGGL(ss_scatter_kernel<true>, dim3(a.num_ranges1), dim3(SS_SBLOCK), 0, s, a);
        return PSS_OK;
    }
    // every first-level bucket counted by its own splitters -> the joint table (the scatter waits for the verdict)
    int second_digits()
    {
        second_ranges();
        a.in = static_cast<const E16 *>(buf.A[0]);
        a.out = static_cast<E16 *>(buf.A[1]);
        hipLaunchKernelGGL(ss_digits2_kernel, dim3((u32)w.max_ranges2), dim3(SS_DBLOCK), 0, s, a);
        joint_offsets();
        return PSS_OK;
    }
    // HOST WAIT: buckets and the largest.  *go = false: a bucket beyond a tile (a sampling accident, probability ~1e-10
    // per bucket: the caller falls back)
    int wait_for_counts(bool *go)
    {
        PSS_TRY(copy_bucket_counts());
        PSS_HIP(hipStreamSynchronize(s));
        take_bucket_counts();
        if (stats) {
            stats->buckets = ne;
            stats->max_bucket = max_bucket;
            stats->b1 = g.B1;
            stats->b2 = g.B2;
            stats->samples = S;
            stats->key_chars = g.kc;
        }
        *go = max_bucket <= SS_MAX_BUCKET;
        if (!*go && debug) explain_refusal();
        return PSS_OK;
    }
    // PSS_SS_DEBUG: where did the crowded bucket come from?  (first-level bucket sizes, the largest joint buckets)
    void explain_refusal() const
    {
        std::vector<u32> hj1(MSD_BINS + 1), hj((size_t)nbk + 1);
        (void)hipMemcpy(hj1.data(), w.J1, (MSD_BINS + 1) * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hj.data(), w.J, ((size_t)nbk + 1) * 4, hipMemcpyDeviceToHost);
        u32 m1 = 0, a1 = 0;
        for (u32 i = 0; i < g.B1; ++i) { const u32 c = hj1[i + 1] - hj1[i]; if (c > m1) { m1 = c; a1 = i; } }
        fprintf(stderr, "[pss] ss declined: n=%u S=%u B1=%u B2=%u kc=%d ib=%d | largest first-level bucket %u (#%u, average %u) | joint buckets above the cap:", n, S,
                g.B1, g.B2, g.kc, g.ib, m1, a1, n / g.B1);
        int shown = 0;
        for (u64 i = 0; i < nbk && shown < 12; ++i) {
            const u32 c = hj[i + 1] - hj[i];
            if (c > SS_MAX_BUCKET) { fprintf(stderr, " #%llu:%u@%u", (unsigned long long)i, c, hj[i]); ++shown; }
        }
        fprintf(stderr, "\n");
    }
    // A[0] -> A[1], every first-level bucket by its own splitters
    void second_scatter() { hipLaunchKernelGGL(ss_scatter_kernel<false>, dim3((u32)w.max_ranges2), dim3(SS_SBLOCK), 0, s, a); }
    // Greedy plan (ss_sort_impl.h).  Its tables live in the first element buffer, which the second scatter has read: at
    // most 3 + levels rows of ne + 1 words, ne < n / 256 (ss_geometry) and levels <= 15 -- under n / 3 of its 16 n bytes.
    // HOST WAIT on the padded route (seg): the padded total decides the number of plan segments.
    int plan_greedy()
    {
        const size_t row = (size_t)ne + 1;
        u32 *pl = reinterpret_cast<u32 *>(buf.A[0]);
        const u32 *starts = w.cstart;
        u32 total = n, cap = SS_TILE_CAP;
        if (seg) {
            // bucket-by-bucket local sort (ss_local_seg_kernel): the plan counts every bucket's length rounded up to eight
            PSS_TRY(device_excl_scan(ctx, InPad8{w.cstart, ne, n}, ne, w.partial, w.d_total(), w.ranks));
            PSS_HIP(hipMemcpyAsync(&h->total, w.d_total(), 8, hipMemcpyDeviceToHost, s));
            pstart = pl;                                                  // the first row of the tables
            hipLaunchKernelGGL(ss_pad_starts_kernel, dim3((u32)((row + 255) / 256)), dim3(256), 0, s, (const u64 *)w.ranks, (const u64 *)w.d_total(), ne,
                               pstart);
            PSS_HIP(hipStreamSynchronize(s));
            total = h->total;
            starts = pstart;
            cap = SS_TILE;
            pl += round_up(row, 64);
        }
        const u32 nseg = (u32)(((u64)total + SS_PLAN_SEG - 1) / SS_PLAN_SEG);
        u32 levels = 0;
        while ((1u << levels) < nseg) ++levels;
        u32 *nxt = pl, *heads = pl + row, *jumps = pl + 2 * row;          // jumps: `levels` rows (at least one)
        const u32 gb = (u32)((row + 255) / 256);
        PSS_HIP(hipMemsetAsync(heads, 0, row * 4, s));
        hipLaunchKernelGGL(ss_plan_next_kernel, dim3(gb), dim3(256), 0, s, starts, ne, total, cap, nxt);
        hipLaunchKernelGGL(ss_plan_exit_kernel, dim3(gb), dim3(256), 0, s, starts, ne, (const u32 *)nxt, jumps);
        for (u32 i = 1; i < levels; ++i)
            hipLaunchKernelGGL(ss_plan_double_kernel, dim3(gb), dim3(256), 0, s, (const u32 *)(jumps + (size_t)(i - 1) * row), (u32)row,
                               jumps + (size_t)i * row);
        hipLaunchKernelGGL(ss_plan_mark_kernel, dim3((nseg + 255) / 256), dim3(256), 0, s, starts, ne, (const u32 *)nxt,
                           (const u32 *)jumps, levels, nseg, heads);
        PSS_TRY(device_excl_scan(ctx, InU32{heads}, ne, w.partial, w.d_total(), w.ranks));
        hipLaunchKernelGGL(ss_plan_tiles_kernel, dim3(1024), dim3(256), 0, s, (const u32 *)heads, ne, (const u64 *)w.ranks,
                           (const u64 *)w.d_total(), w.tile_first);
        return PSS_OK;
    }
    // Ties go out as flags (bit 31 = "same key as my predecessor", the contract of suffix_sort_flags), not as the records
    // of the fused first rerank: groups of equal keys cross tile boundaries here, and the flag of a tile's first element
    // takes a look at the tile before it (ss_boundary_kernel, once every tile is sorted).
    int local_sort()
    {
        PSS_TRY(times.begin(ST_LOCAL));
        if (pstart)
            hipLaunchKernelGGL(ss_local_seg_kernel, dim3(nt), dim3(SL_BLOCK), 0, s, (const E16 *)buf.A[1], (const MsdTile *)w.tiles_all, nt, g.ib,
                               (const u32 *)w.cstart, (const u32 *)pstart, (const u32 *)w.tile_first, ne, n, sa_out);
        else
            hipLaunchKernelGGL(ss_local_kernel, dim3(nt), dim3(SL_BLOCK), 0, s, (const E16 *)buf.A[1], (const MsdTile *)w.tiles_all, nt, g.ib,
                               sa_out);
        return times.end(ST_LOCAL);
    }
    void boundaries() { hipLaunchKernelGGL(ss_boundary_kernel, dim3((nt + 255) / 256), dim3(256), 0, s, (const MsdTile *)w.tiles_all, nt, tx, sa_out); }
    int report()
    {
        if (stats) stats->tiles = nt;
        if (!times.on || !stats) return PSS_OK;
        PSS_HIP(hipStreamSynchronize(s));
        PSS_TRY(times.ms(ST_SAMPLE, &stats->ms_sample));
        PSS_TRY(times.ms(ST_G1, &stats->ms_g1));
        PSS_TRY(times.ms(ST_G2, &stats->ms_g2));
        return times.ms(ST_LOCAL, &stats->ms_local);
    }

    int run(bool *accepted)
    {
        PSS_TRY(times.begin(ST_SAMPLE));
        PSS_TRY(sample());
        PSS_TRY(times.mark(ST_SAMPLE, ST_G1));
        PSS_TRY(first_pass());
        PSS_TRY(times.mark(ST_G1, ST_G2));
        PSS_TRY(second_digits());
        PSS_TRY(count_buckets(nullptr));
        bool go = false;
        PSS_TRY(wait_for_counts(&go));
        if (!go) return PSS_OK;
        second_scatter();
        PSS_TRY(times.end(ST_G2));
        PSS_TRY(window_plan ? plan_windows(TilePlan{SS_WIN, SS_TILE_CAP, nullptr}) : plan_greedy());
        PSS_TRY(wait_for_tiles("ss_suffix_sort"));
        describe_tiles(nullptr);
        PSS_TRY(local_sort());
        boundaries();
        PSS_HIP(hipGetLastError());
        PSS_TRY(report());
        *accepted = true;
        return PSS_OK;
    }
};

int ss_suffix_sort(DeviceCtx *ctx, const TextKeys *text, uint32_t radix, uint32_t n, const SsBuffers &buf, uint32_t *sa_out,
                   void *work, uint32_t *h_small, bool profile, SsStats *stats, bool *accepted)
{
    *accepted = false;
    SsGeometry g;
    if (!ss_geometry(n, radix, &g)) return PSS_OK;      // not this text
    SsSort sort(ctx, text, radix, n, g, buf, sa_out, work, h_small, profile, stats);
    return sort.run(accepted);
}
