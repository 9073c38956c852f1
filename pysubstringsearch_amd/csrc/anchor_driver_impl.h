// anchor_driver_impl.h -- host side of the anchor round (kernels: anchor_impl.h): the driver that selects the anchors, sorts them with rounds of their own and spreads their ranks (AnchorRound), and the side line that runs it beside the text round (side_start).
// Included by sa_build.hip (inside namespace pss, after sa_refine_impl.h): one translation unit, split by route.

// Starts the side line: anchors of the text `codes` for windows that fit depth h_eff, sorted in ctx's helper context.
// after (optional): an event on the main stream that the helper's stream waits for first (the codes are being written).
// No room for the buffers is not an error: the anchors then wait their turn on the main line as before.
static int side_start(DeviceCtx *ctx, const Knobs &knobs, SideAnchors &side, u32 n, const u8 *codes, int b, int plus_one, u64 h_eff,
                      hipEvent_t after)
{
    if (side.started) return PSS_OK;
    DeviceCtx *hc = nullptr;
    const size_t sort_ws = radix_sort_workspace_bytes();
    int rs = get_helper_ctx(ctx, &hc);
    if (rs == PSS_OK) rs = hc->slot[S_K0].reserve((size_t)n * 8);
    if (rs == PSS_OK) rs = hc->slot[S_K1].reserve((size_t)n * 8);
    if (rs == PSS_OK) rs = hc->slot[S_ISA].reserve((size_t)n * 4 + 64);
    if (rs == PSS_OK) rs = hc->slot[S_WORK].reserve(sort_ws + 65536);
    if (rs != PSS_OK) {
        (void)hipGetLastError();
        set_error("%s", "");
        return PSS_OK;
    }
    if (after) PSS_HIP(hipStreamWaitEvent(hc->stream, after, 0));
    u8 *hw = hc->slot[S_WORK].as<u8>();
    // (the string the anchors are chosen from, and the two key buffers their sort may use: all an anchor round reads of its caller)
    RoundsIO o2;
    o2.n = n;
    o2.K[0] = hc->slot[S_K0].as<u64>();
    o2.K[1] = hc->slot[S_K1].as<u64>();
    o2.codes = codes;
    o2.b = b;
    o2.plus_one = plus_one;
    o2.work = hw;
    o2.sm = SmallState(hw + sort_ws, hc->pinned);
    side.h_eff = h_eff;
    side.akey = hc->slot[S_ISA].as<u32>();
    memset(&side.st, 0, sizeof side.st);
    const int dev = ctx->device;
    SideAnchors *sp = &side;
    // (std::thread's constructor may throw -- no more threads to be had: the flag goes up only once the thread exists, so
    // that the destructor never joins what was never started; the exception travels to the C ABI's catch-all)
    side.th = std::thread([hc, knobs, o2, h_eff, sp, dev]() {
        if (hipSetDevice(dev) != hipSuccess) {
            sp->rc = PSS_EDEVICE;
            sp->err = "hipSetDevice failed in the anchors' side line";
            return;
        }
        try {
            sp->rc = anchor_rank_keys(hc, knobs, o2, h_eff, nullptr, nullptr, sp->akey, sp->st, &sp->ok);
            if (sp->rc != PSS_OK) sp->err = last_error();
        } catch (const std::bad_alloc &) {
            sp->rc = PSS_ENOMEM;
            sp->err = "host allocation failed in the anchors' side line";
        } catch (...) {                      // (nothing may leave a thread's function)
            sp->rc = PSS_EDEVICE;
            sp->err = "internal error in the anchors' side line";
        }
    });
    side.started = true;
    return PSS_OK;
}

__global__ __launch_bounds__(256) void gather_names_kernel(const u32 *pos, u32 m, const u32 *ranks, u64 *keys, u32 *vals)
{
    for (u32 t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        keys[t] = ranks[pos[t]];
        vals[t] = t;
    }
}

// The key of the anchor round (anchor_impl.h): akey[i] = rank, among the anchor suffixes, of the anchor the window at i
// chose -- for every position i of the string.  `h`: symbols every tied group of the caller's active list shares.
//   syms == nullptr  the string is the text (outer.codes): w = 4 or 8 bytes hashed per position, omega + w - 1 <= h; the
//                    anchors are named by a sort of their own (text rounds to 2 omega + w - 1 symbols), then their names
//                    are a string of 32-bit symbols whose suffixes the rank rounds sort;
//   syms != nullptr  the string is that array of 32-bit symbols (a level up: the names of a coarser level's anchors):
//                    w = 1, omega = h / 2, and the anchors' names are the ranks the caller's rounds have reached
//                    (cur_ranks, depth h >= 2 omega).
// The caller's key buffers K[0], K[1] (8 n bytes each, scratch between two rounds) hold the anchors' own sort; `akey`:
// 4 n bytes (may be cur_ranks).  *ok = false: declined (window too narrow, too many anchors) -- nothing is lost but the
// time of the selection pass.
// run(): window -> select (the anchors counted and listed) -> sort_anchors (rounds of their own, a level down) -> spread.
struct AnchorRound {
    DeviceCtx *const ctx;
    const Knobs &knobs;
    const RoundsIO &outer;
    const u64 h;
    const u32 *const syms, *const cur_ranks;
    u32 *const akey;
    pss_sa_stats &st;
    hipStream_t s;
    const u32 n;
    int w = 0;
    u32 omega = 0;
    u32 cap_div = 5, num_tiles = 0, grid = 0;
    u8 *d_dist = nullptr;
    u32 *d_tile_cnt = nullptr, *d_Q = nullptr;
    u64 *d_tile_off = nullptr;
    u32 m = 0;                  // anchors
    u32 *A_sa = nullptr, *A_rank = nullptr;
    BuildTimer tm;

    AnchorRound(DeviceCtx *ctx_, const Knobs &knobs_, const RoundsIO &outer_, u64 h_, const u32 *syms_, const u32 *cur_ranks_, u32 *akey_,
                pss_sa_stats &st_)
        : ctx(ctx_), knobs(knobs_), outer(outer_), h(h_), syms(syms_), cur_ranks(cur_ranks_), akey(akey_), st(st_), s(ctx_->stream), n(outer_.n)
    {
    }

    int run(bool *ok)
    {
        *ok = false;
        if (!window()) return PSS_OK;
        bool go = false;
        PSS_TRY(select(&go));
        if (!go) return PSS_OK;
        PSS_TRY(sort_anchors(&go));
        if (!go) return PSS_OK;
        PSS_TRY(spread());
        *ok = true;
        return PSS_OK;
    }

    // How wide the windows may be at this depth; false: too narrow (or too small a string, too many levels).
    bool window()
    {
        const bool forced = knobs.anchor == 1;
        u64 omega64;
        if (syms) {
            w = 1;
            omega64 = h / 2;
        } else {
            w = h >= 28 ? 8 : 4;
            omega64 = h >= (u64)w ? h - (u64)w + 1 : 0;
        }
        if (knobs.anchor_omega > 0) omega64 = std::min<u64>(omega64, (u64)knobs.anchor_omega);
        omega = (u32)std::min<u64>(omega64, 64);       // wider windows: fewer anchors, but names of 2 omega + w - 1 symbols
        return !(omega < (forced ? 2u : (u32)knobs.anchor_min_omega) || n < 64 || outer.level >= 6);
    }

    // The anchors chosen, counted (one wait) and -- unless there are none or too many -- listed in Q.
    int select(bool *go)
    {
        *go = false;
        cap_div = outer.level == 0 ? (u32)knobs.anchor_cap_div : 5u;
        const AnchorScratch A(n, cap_div);
        num_tiles = A.num_tiles;
        DevBuf &slot = ctx->slot[S_ANC + outer.level];
        PSS_TRY(slot.reserve(A.reserved()));
        u8 *base = slot.as<u8>();
        d_dist = base + A.dist;
        d_tile_cnt = region<u32>(base, A.tile_cnt);
        d_tile_off = region<u64>(base, A.tile_off);
        u64 *d_partial = region<u64>(base, A.partial), *d_total = d_partial + AnchorScratch::TOTAL_AT;
        d_Q = region<u32>(base, A.Q);
        PSS_HIP(hipEventCreate(&tm.ev0));
        PSS_HIP(hipEventCreate(&tm.ev1));
        PSS_HIP(hipEventRecord(tm.ev0, s));
        const u32 n_read = (u32)(round_up((size_t)n, 16) + 64);      // the recoded text's padding (zero)
        grid = std::min<u32>(num_tiles, (u32)ctx->num_cus * 4);
        if (syms)
            hipLaunchKernelGGL(anc_select_kernel<true>, dim3(grid), dim3(256), 0, s, reinterpret_cast<const u8 *>(syms), n, n, omega, w,
                               d_dist, d_tile_cnt, num_tiles);
        else
            hipLaunchKernelGGL(anc_select_kernel<false>, dim3(grid), dim3(256), 0, s, outer.codes, n, n_read, omega, w, d_dist, d_tile_cnt,
                               num_tiles);
        PSS_TRY(device_excl_scan(ctx, InU32{d_tile_cnt}, num_tiles, d_partial, d_total, d_tile_off));
        u32 *h_small = outer.sm.h_small;
        PSS_HIP(hipMemcpyAsync(h_small, d_total, 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        m = h_small[0];
        if (outer.level == 0) {
            st.anchor_count = m;
            st.anchor_omega = omega;
            st.anchor_w = (u64)w;
        }
        if (knobs.timing)
            fprintf(stderr, "[pss] anchors (level %d): n=%u h=%llu omega=%u w=%d anchors=%u (n / %.1f)\n", outer.level, n,
                    (unsigned long long)h, omega, w, m, (double)n / std::max(1u, m));
        if (m == 0 || m > n / cap_div) return PSS_OK;
        hipLaunchKernelGGL(anc_walk_kernel<false>, dim3(grid), dim3(256), 0, s, d_dist, n, d_tile_off, num_tiles, d_Q,
                           (const u32 *)nullptr, (u32 *)nullptr);
        *go = true;
        return PSS_OK;
    }

    // The anchors' own sort, in the caller's two key buffers (AnchorSort): initial keys, one radix sort, then Rounds a
    // level down -- in subset mode over the text, or over the names the caller's ranks give them.
    int sort_anchors(bool *go)
    {
        *go = false;
        const AnchorSort A(n, m, outer.level);
        if (A.where == AnchorSort::decline) return PSS_OK;
        u8 *b0 = reinterpret_cast<u8 *>(outer.K[0]), *b1 = reinterpret_cast<u8 *>(outer.K[1]);
        if (A.where == AnchorSort::own_slot) {
            PSS_TRY(ctx->slot[S_ANCW].reserve(A.second_bytes));
            b1 = ctx->slot[S_ANCW].as<u8>();
        }
        u64 *AK[2] = {region<u64>(b0, A.AK[0]), region<u64>(b0, A.AK[1])};
        u32 *AV[2] = {region<u32>(b1, A.AV[0]), region<u32>(b1, A.AV[1])};
        A_sa = region<u32>(b1, A.sa);
        A_rank = region<u32>(b1, A.rank);
        const int kt = symbols_per_key(outer.b);
        const u32 gk = (u32)std::min<u64>((u64)ctx->num_cus * 8, ((u64)m + 255) / 256);
        int cur = 0;
        SortStats ss;
        RoundsIO io;
        if (syms) {
            hipLaunchKernelGGL(gather_names_kernel, dim3(gk), dim3(256), 0, s, d_Q, m, cur_ranks, AK[0], AV[0]);
            PSS_TRY(radix_sort_pairs(ctx, AK, AV, m, rank_bits(n), 0xffffffffu, nullptr, 0, outer.work, &cur, false, &ss));
            io = RoundsIO::for_integers(outer.sm, outer.work, m, A_sa, AK, AV, region<u32>(b1, A.isa), region<u32>(b1, A.AP[0]),
                                        region<u32>(b1, A.AP[1]), region<u32>(b1, A.grp));
        } else {
            hipLaunchKernelGGL(subset_keys_kernel, dim3(gk), dim3(256), 0, s, d_Q, m, n, outer.codes, outer.b, kt, outer.plus_one, AK[0], AV[0]);
            PSS_TRY(radix_sort_pairs(ctx, AK, AV, m, kt * outer.b, 0xffffffffu, nullptr, 0, outer.work, &cur, false, &ss));
            io = RoundsIO::for_text(outer.sm, outer.work, m, A_sa, AK, AV, region<u32>(b1, A.isa), region<u32>(b1, A.AP[0]),
                                    region<u32>(b1, A.AP[1]), region<u32>(b1, A.grp), outer.codes, outer.b, outer.plus_one, kt, 0);
            io.sub_pos = d_Q;
            io.text_n = n;
            io.stop_text_h = 2ull * omega + (u64)w - 1;
        }
        io.grp2 = region<u32>(b1, A.grp2);
        io.cur = cur;
        io.no_sparse = true;
        io.level = outer.level + 1;
        pss_sa_stats sub;
        memset(&sub, 0, sizeof sub);
        SortStats ss2;
        PSS_TRY(Rounds(ctx, knobs, io, ss2, sub).run());
        st.anchor_text_rounds += sub.text_rounds;
        st.anchor_rounds += sub.rounds - sub.text_rounds + sub.anchor_rounds;
        st.anchor_sum_active += sub.sum_active + sub.anchor_sum_active;
        st.anchor_left += sub.anchor_left;
        st.periodic_rounds += sub.periodic_rounds;
        st.periodic_members += sub.periodic_members;
        st.anchor_levels = std::max<uint64_t>(st.anchor_levels, 1 + sub.anchor_levels);
        *go = true;
        return PSS_OK;
    }

    // Every position gets the rank of the anchor its window chose.
    int spread()
    {
        const u32 gk = (u32)std::min<u64>((u64)ctx->num_cus * 8, ((u64)m + 255) / 256);
        hipLaunchKernelGGL(isa_from_sa_kernel, dim3(gk), dim3(256), 0, s, A_sa, m, A_rank);
        hipLaunchKernelGGL(anc_walk_kernel<true>, dim3(grid), dim3(256), 0, s, d_dist, n, d_tile_off, num_tiles, (u32 *)nullptr,
                           (const u32 *)A_rank, akey);
        PSS_HIP(hipEventRecord(tm.ev1, s));
        PSS_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        PSS_HIP(hipEventElapsedTime(&ms, tm.ev0, tm.ev1));
        if (outer.level == 0) {
            st.anchor_ms += ms;
            st.anchor_depth = h;
        }
        st.anchor = 1;
        return PSS_OK;
    }
};

static int anchor_rank_keys(DeviceCtx *ctx, const Knobs &knobs, const RoundsIO &outer, u64 h, const u32 *syms,
                            const u32 *cur_ranks, u32 *akey, pss_sa_stats &st, bool *ok)
{
    return AnchorRound(ctx, knobs, outer, h, syms, cur_ranks, akey, st).run(ok);
}
