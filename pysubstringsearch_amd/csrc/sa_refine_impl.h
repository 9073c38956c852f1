// sa_refine_impl.h -- host side of everything after the initial sort: the rounds (Rounds).  The anchor round's driver and its side line follow in anchor_driver_impl.h.
// Included by sa_build.hip (inside namespace pss, after the alphabet kernels): one translation unit, split by route.

static_assert(ROUNDS_SCAN_BLOCKS == SC_MAX_BLOCKS, "rounds_layout.h restates the partial sums of scan.h");

// The 64 KiB of small device state that follow the radix sort's workspace in slot S_WORK of a context, and the pinned
// host scratch its counters are read through.
struct SmallState {
    u32 *present = nullptr, *counts = nullptr;      // [256] byte values that occur, [256] their sampled counts (one 2048-byte block)
    u8 *lut = nullptr;                              // [256] byte -> code
    u32 *agg_head = nullptr, *agg_cnt = nullptr;    // [1024] each
    u64 *red = nullptr;                             // [2]
    u32 *counters = nullptr;                        // the rounds' own cells, and behind them:
    u32 *tied = nullptr;                            // [16] tied counts of the sizing sample
    u32 *runs = nullptr, *dups = nullptr;           // runs of equal bytes | sampled places seen before (neighbours: one copy fetches both)
    u32 *bad = nullptr;                             // a byte of the text had no code in the table the MSD sort was given
    u32 *h_small = nullptr;
    SmallState() = default;     // (a Build's, before carve())
    SmallState(u8 *small, void *pinned)
        : present(reinterpret_cast<u32 *>(small)), counts(present + 256), lut(small + 2048),
          agg_head(reinterpret_cast<u32 *>(small + 4096)), agg_cnt(reinterpret_cast<u32 *>(small + 8192)),
          red(reinterpret_cast<u64 *>(small + 12288)), counters(reinterpret_cast<u32 *>(small + 12288 + 64)), tied(counters + 16),
          runs(counters + 40), dups(counters + 41), bad(counters + 44), h_small(static_cast<u32 *>(pinned))
    {
    }
};

// Everything after the initial sort: rerank + compaction of the tied suffixes, then rounds until no
// ties are left.  Its own driver since round 2: the run-length path (rle_build.hip) sorts the
// suffixes of an INTEGER string (one symbol per run of the text) with the same rounds -- there is no
// text to pack keys from then (codes == nullptr): rank rounds only, starting from h0 = 1.
// What the rounds are given.  The two makers fill what every caller has to say; the rest keeps its default until a
// caller names it.
struct RoundsIO {
    u32 n = 0;
    u32 *SA = nullptr;
    u64 *K[2] = {nullptr, nullptr};
    u32 *V[2] = {nullptr, nullptr};
    u32 *ISA = nullptr;
    u32 *P[2] = {nullptr, nullptr};
    u32 *GRP = nullptr;
    const u8 *codes = nullptr;  // recoded text (nullptr: rank rounds only)
    int b = 8, plus_one = 0, key_chars = 1, key_drop = 0;
    u64 h0 = 1;                 // symbols every group of the initial sort is known to share
    int cur = 0;                // K[cur] / V[cur]: sorted keys / suffixes of the initial sort
    int final_buf = -1;         // V[final_buf] was redirected to SA for the initial sort (-1: not)
    u32 *v_scratch = nullptr;   // ... and this is the buffer it stands for
    bool ties = false;          // V[cur] carries tie flags in bit 31 (no keys)
    bool msd_fused = false;     // the MSD sort already produced the first active list
    u32 msd_active = 0;
    bool no_sparse = false;     // the initial key does not fit 64 bits (sample sort): the sparse mode's key search cannot be used
    u8 *work = nullptr;         // the radix sort's workspace ...
    SmallState sm;              // ... and the small state behind it
    bool profile = false;
    // Subset sort (anchors, anchor_impl.h): the n elements are the suffixes at text positions sub_pos[0 .. n) of a text of
    // text_n symbols; element values are the ordinals.  Text rounds run until every group shares stop_text_h symbols,
    // whatever they resolve; then the group ranks are the symbols of an integer string (element v is followed by v + 1)
    // whose suffixes the rank rounds sort, starting over from h = 1.
    const u32 *sub_pos = nullptr;
    u32 text_n = 0;
    u64 stop_text_h = 0;
    u32 *grp2 = nullptr;        // second group-rank buffer (nullptr: slot S_GRP2 of the context)
    int level = 0;              // 0: the text (or the run-length path's reduced string); k: the names of level k - 1's anchors
    struct SideAnchors *side = nullptr;      // the side line of the build these rounds belong to (it may be under way already)

    // The suffixes of an integer string of n symbols: rank rounds only, from depth 1.
    static RoundsIO for_integers(const SmallState &sm, u8 *work, u32 n, u32 *SA, u64 *const K[2], u32 *const V[2], u32 *ISA, u32 *P0,
                                 u32 *P1, u32 *GRP)
    {
        RoundsIO io;
        io.n = n;
        io.SA = SA;
        io.K[0] = K[0]; io.K[1] = K[1];
        io.V[0] = V[0]; io.V[1] = V[1];
        io.ISA = ISA;
        io.P[0] = P0; io.P[1] = P1;
        io.GRP = GRP;
        io.work = work;
        io.sm = sm;
        return io;
    }
    // Suffixes of the recoded text, sorted by their first key_chars symbols (the last one short of key_drop bits).
    static RoundsIO for_text(const SmallState &sm, u8 *work, u32 n, u32 *SA, u64 *const K[2], u32 *const V[2], u32 *ISA, u32 *P0, u32 *P1,
                             u32 *GRP, const u8 *codes, int b, int plus_one, int key_chars, int key_drop)
    {
        RoundsIO io = for_integers(sm, work, n, SA, K, V, ISA, P0, P1, GRP);
        io.codes = codes;
        io.b = b; io.plus_one = plus_one; io.key_chars = key_chars; io.key_drop = key_drop;
        io.h0 = (u64)(key_drop ? key_chars - 1 : key_chars);
        return io;
    }
};

// The anchors' own sort BESIDE the text round (round 5).  Which positions are anchors, their names and the order of the
// anchor suffixes depend on the text and on the window only -- not on the active list the text round is busy with.  On
// text with copies in it (source code: 412 MB of real files spent 34 ms in the text round and 50 ms in the anchors'
// sort, one after the other) the anchors are therefore sorted by a second host thread on a second stream, in a context
// of its own (DeviceCtx::helper: its stream, pinned scratch and slots), while the main line runs the text round that
// raises the depth to what the window needs.  Half of the anchors' sort is a long row of small launches (rank rounds over
// lists of 10^4 .. 10^6 elements on three levels) that leave the device all but empty: they fill the gaps of the other
// stream instead of standing in line.  The window is fixed in advance (the depth the text round WILL reach); a text round
// that gives up half-way leaves the depth where it was, and the result of the side line is then thrown away.
struct SideAnchors {
    std::thread th;
    bool started = false, joined = false, ok = false;
    int rc = PSS_OK;
    std::string err;
    u64 h_eff = 0;
    pss_sa_stats st;
    u32 *akey = nullptr;
    void join()
    {
        if (started && !joined) {
            if (th.joinable()) th.join();
            joined = true;
        }
    }
    ~SideAnchors() { join(); }
};

// (anchor_driver_impl.h)
static int anchor_rank_keys(DeviceCtx *ctx, const Knobs &knobs, const RoundsIO &outer, u64 h, const u32 *syms,
                            const u32 *cur_ranks, u32 *akey, pss_sa_stats &st, bool *ok);
static int side_start(DeviceCtx *ctx, const Knobs &knobs, SideAnchors &side, u32 n, const u8 *codes, int b, int plus_one, u64 h_eff,
                      hipEvent_t after);

template <typename T> static T *region(u8 *base, size_t offset) { return reinterpret_cast<T *>(base + offset); }

// One group-local round over the active list (Rounds::local_round): its scratch and what its stages hand on.
struct LocalRound {
    const bool use_text;            // keys from the text | from ranks
    const u32 *const key_of_suffix; // anchor round: the key of suffix i is key_of_suffix[i] (the rank of the anchor its window chose)
    const u32 h32;
    const RoundScratch L;
    u8 *d_big = nullptr;            // [m] member of a large group
    u32 *d_blk_big = nullptr, *d_blk_heads = nullptr;      // [nblk] flagged members | flagged heads per window
    u64 *d_off_big = nullptr, *d_off_heads = nullptr, *d_partial = nullptr, *d_total = nullptr;
    u32 nbig = 0, nbig_groups = 0;
    // the large groups, compacted (BigScratch)
    u32 *d_bt = nullptr, *d_bgid = nullptr;
    u64 *BK[2] = {nullptr, nullptr};
    u32 *BV[2] = {nullptr, nullptr};
    int gid_bits = 1, big_key_bits = 0;
    LocalRound(bool text, const u32 *key, u64 h, u32 m, bool mid_tier)
        : use_text(text), key_of_suffix(key), h32((u32)std::min<u64>(h, 0xffffffffull)), L(m, mid_tier)
    {
    }
    void bind(u8 *scr)
    {
        d_big = scr + L.big;
        d_blk_big = region<u32>(scr, L.blk_big);
        d_blk_heads = region<u32>(scr, L.blk_heads);
        d_off_big = region<u64>(scr, L.off_big);
        d_off_heads = region<u64>(scr, L.off_heads);
        d_partial = region<u64>(scr, L.partial);
        d_total = d_partial + RoundScratch::TOTAL_AT;
    }
};

// The rounds of one sort, staged: run() reads top to bottom.  Every round reranks the sorted list (rerank_count gives
// the suffixes still tied; round 0 chooses the mode from them; rerank_apply writes the ranks and compacts the active
// list), checks that progress is possible, and takes ONE of: a text round or the anchor round in its place
// (text_stage), an anchor round a level up (level_up), a group-local rank round (rank_round), a global one
// (global_round).  The members are the state the rounds share.
struct Rounds {
    enum class Took { nothing, anchor, text, rank };      // which round ran: h stays | advances by kt | doubles

    DeviceCtx *const ctx;
    const Knobs &knobs;
    const RoundsIO &io;
    SortStats &ss;
    pss_sa_stats &st;
    hipStream_t s;
    const u32 n;
    u32 *const SA;
    u64 *K[2];
    u32 *V[2];
    u32 *const ISA;
    u32 *P[2];
    u32 *G[2];
    const u8 *const codes;
    const bool rank_only, subset;
    const u32 text_n;
    const int b, plus_one;
    const int kt;                // symbols per text-round key
    const int rbits;             // bits of a rank 0..n
    u32 *const h_small;
    const int grid_stream;
    const u32 grid_all;
    const bool sa_in_place;
    RerankArgs ra;
    // the list and where it lies
    int round = 0;
    u32 m, m_next = 0;
    int cur;
    int pcur = 0;                // P[pcur] holds the SA positions of the active list (after round 0)
    int gcur = 0;                // G[gcur] holds its group ranks
    int src = 0;                 // V[src] = compacted suffix indices, G[gcur] their groups, P[pcur] their slots
    u32 grid = 0;
    bool identity_pos = true;
    const int k0buf;             // K[k0buf] = sorted initial keys (kept intact in sparse mode)
    u64 *SK[2] = {nullptr, nullptr};   // sparse mode: small ping-pong key buffers
    u64 **Kr = K;
    // what the rounds have learnt
    RoundMode mode = M_DENSE;
    bool was_text = false;
    int text_rounds = 0;
    u32 m_text_prev = 0;
    bool keyed_grp = true;       // the sorted keys of the previous round carry the group rank in their high half
    u32 global_above = 0;        // rank rounds use ONE global (group, rank) sort while m stays above this
    double last_big_frac = 0.0;
    u64 h;                       // symbols every group is known to share
    bool anchored = false;       // the anchor round has run: nothing may be left tied
    SideAnchors own_side;
    SideAnchors &side;
    // Integer strings (rank rounds only): the ranks the first round leaves ARE the string, up to renaming -- kept for the
    // minimizers of an anchor level on top of this one (anchor_impl.h), should the rounds reach depth 32 with much left tied.
    u32 *X0 = nullptr;
    const u32 *Xsym = nullptr;   // the same snapshot for the periodic keys of the rank rounds (per_*_kernel), never given up
    bool last_per = false;       // the last rank round met periodic runs among its large groups, or chains that will be
    u64 per_wait_h = 0;          // ... and the depth from which their period can be seen

    Rounds(DeviceCtx *ctx_, const Knobs &knobs_, const RoundsIO &io_, SortStats &ss_, pss_sa_stats &st_)
        : ctx(ctx_), knobs(knobs_), io(io_), ss(ss_), st(st_), s(ctx_->stream), n(io_.n), SA(io_.SA), K{io_.K[0], io_.K[1]},
          V{io_.V[0], io_.V[1]}, ISA(io_.ISA), P{io_.P[0], io_.P[1]}, G{io_.GRP, nullptr}, codes(io_.codes), rank_only(io_.codes == nullptr),
          subset(io_.sub_pos != nullptr), text_n(subset ? io_.text_n : io_.n), b(io_.b), plus_one(io_.plus_one), kt(symbols_per_key(io_.b)),
          rbits(rank_bits(io_.n)), h_small(io_.sm.h_small), grid_stream(ctx_->num_cus * 8), grid_all((u32)grid_stream),
          sa_in_place(io_.final_buf >= 0 && io_.cur == io_.final_buf), m(io_.n), cur(io_.cur), k0buf(io_.cur), h(io_.h0),
          side(io_.side ? *io_.side : own_side)
    {
        memset(&ra, 0, sizeof ra);
        ra.agg_head = io.sm.agg_head;
        ra.agg_cnt = io.sm.agg_cnt;
        ra.SA = SA;
        ra.ISA = ISA;
        ra.counters = io.sm.counters;
        ra.ht = reinterpret_cast<u64 *>(ISA);     // the two modes never coexist
        ra.rank_bits = rbits;
    }
    Rounds(const Rounds &) = delete;

    int run()
    {
        for (round = 0;; ++round) {
            if (round > 96) {
                set_error("sa_build: no convergence after 96 rounds (internal error)");
                return PSS_EDEVICE;
            }
            PSS_TRY(rerank_count());
            if (round == 0) choose_mode();
            PSS_TRY(rerank_apply());
            if (m_next == 0) break;
            PSS_TRY(check_progress());
            enter_round();
            Took took = Took::nothing;
            if (mode == M_TEXT) PSS_TRY(text_stage(&took));
            if (took == Took::nothing) PSS_TRY(level_up(&took));
            if (took == Took::nothing) PSS_TRY(rank_round(&took));
            if (took == Took::nothing) PSS_TRY(global_round());
        }
        st.mode = was_text ? (mode == M_TEXT ? 2u : 3u) : (u64)mode;
        return PSS_OK;
    }

    // ---- rerank ----
    bool fused0() const { return round == 0 && io.msd_fused; }     // the MSD local sort already produced this round's active list

    // Where the sorted list lies and where the active list goes; the suffixes still tied (m_next).
    int rerank_count()
    {
        rerank_geometry(m, ra);
        ra.keys = Kr[cur];
        ra.idx = V[cur];
        ra.SA = (round == 0 && sa_in_place) ? nullptr : SA;      // round 0: the sort already wrote SA
        ra.tied_sa = (round == 0 && io.ties && !io.msd_fused) ? V[cur] : nullptr;
        ra.pos = identity_pos ? nullptr : P[pcur];
        ra.grp = (round > 0 && !keyed_grp) ? G[gcur] : nullptr;   // group-local rounds: keys do not carry the group
        ra.pos_out = P[pcur ^ 1];
        ra.idx_out = V[cur ^ 1];
        if (round == 0) {
            if (io.grp2) G[1] = io.grp2;
            else {
                PSS_TRY(ctx->slot[S_GRP2].reserve((size_t)n * 4));
                G[1] = ctx->slot[S_GRP2].as<u32>();
            }
        }
        ra.grp_out = G[gcur ^ 1];
        if (!fused0()) {
            if (ra.tied_sa) hipLaunchKernelGGL(rr_reduce_tied_kernel, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
            else hipLaunchKernelGGL(rr_reduce_kernel, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
            hipLaunchKernelGGL(rr_scan_kernel, dim3(1), dim3(1024), 0, s, io.sm.agg_head, io.sm.agg_cnt, ra.num_ranges, io.sm.counters);
            PSS_HIP(hipMemcpyAsync(h_small, io.sm.counters, 4, hipMemcpyDeviceToHost, s));
            PSS_HIP(hipStreamSynchronize(s));
        }
        m_next = fused0() ? io.msd_active : h_small[0];
        return PSS_OK;
    }

    void choose_mode()
    {
        mode = first_mode(n, m_next, h, knobs.mode, knobs.text_rounds_max, rank_only, subset, io.no_sparse, io.stop_text_h);
        was_text = mode == M_TEXT;
    }

    int rerank_apply()
    {
        if (fused0()) {
            if (mode == M_DENSE && m_next) {      // rank rounds from the start: they need the inverse suffix array
                hipLaunchKernelGGL(isa_from_sa_kernel, dim3(grid_all), dim3(256), 0, s, SA, n, ISA);
                hipLaunchKernelGGL(isa_active_kernel, dim3(grid_all), dim3(256), 0, s, ra.idx_out, ra.grp_out, m_next, ISA);
            }
        } else if (mode == M_DENSE) hipLaunchKernelGGL(rr_apply_kernel<MODE_ISA>, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
        else if (mode == M_SPARSE && round > 0) hipLaunchKernelGGL(rr_apply_kernel<MODE_HT>, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
        else if (ra.tied_sa && ra.SA == nullptr && ra.pos == nullptr)
            hipLaunchKernelGGL(rr_apply_tied_kernel, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
        else hipLaunchKernelGGL(rr_apply_kernel<MODE_NONE>, dim3(ra.num_ranges), dim3(RR_BLOCK), 0, s, ra);
        PSS_HIP(hipGetLastError());
        if (round == 0 && io.final_buf >= 0) V[io.final_buf] = io.v_scratch;   // later rounds must not scribble over SA
        return PSS_OK;
    }

    int snapshot_symbols()
    {
        const bool for_levels = !(knobs.anchor == 0 || io.level >= 6 || n < (knobs.anchor == 1 ? 64u : (1u << 20)));
        if (!for_levels && (knobs.no_periodic || io.level >= 6 || n <= 3072u)) return PSS_OK;
        PSS_TRY(ctx->slot[S_X0 + io.level].reserve((size_t)n * 4));
        u32 *snap = ctx->slot[S_X0 + io.level].as<u32>();
        PSS_HIP(hipMemcpyAsync(snap, ISA, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        if (for_levels) X0 = snap;
        Xsym = snap;
        return PSS_OK;
    }

    // The two exits that cannot happen, and what a sort that starts with rank rounds keeps of its first ranks.
    int check_progress()
    {
        if (anchored && mode == M_DENSE) {
            // cannot happen: the anchor round leaves no ties (and its keys took the place of the inverse array)
            st.anchor_left += m_next;
            set_error("sa_build: %u elements tied after the anchor round of level %d (internal error)", m_next, io.level);
            return PSS_EDEVICE;
        }
        if (round == 0 && mode == M_DENSE && subset) h = 1;           // (no text round was needed: the elements are symbols already)
        if (round == 0 && mode == M_DENSE && (subset || rank_only)) PSS_TRY(snapshot_symbols());
        // (subset mode counts h in SYMBOLS of the text while its text rounds run, in elements afterwards)
        if (h >= (subset && mode == M_TEXT ? (u64)text_n : (u64)n)) {
            set_error("sa_build: %u suffixes unresolved at h=%llu >= n (internal error)", m_next,
                      (unsigned long long)h);
            return PSS_EDEVICE;
        }
        return PSS_OK;
    }

    void enter_round()
    {
        m = m_next;
        pcur ^= 1;
        gcur ^= 1;
        identity_pos = false;
        src = cur ^ 1;
        grid = (u32)std::min<u64>((u64)grid_stream, ((u64)m + 255) / 256);
    }

    // The round is done: its output is the sorted list of the next rerank.
    int took_round(Took kind, Took *took)
    {
        keyed_grp = false;
        cur = src ^ 1;
        st.rounds += 1;
        if (kind == Took::text) {
            st.text_rounds += 1;
            text_rounds += 1;
        }
        st.sum_active += m;
        if (kind == Took::text) h += (u64)kt;
        if (kind == Took::rank) h *= 2;
        PSS_HIP(hipGetLastError());
        *took = kind;
        return PSS_OK;
    }

    // ------------------------------------------------------ group-local round --
    // One round over the active list: a 64-bit key per suffix, every group sorted by it.
    //   text round : key = next symbols packed from the text at offset h      (h += kt)
    //   rank round : key = rank of suffix i+h from the inverse suffix array    (h *= 2)
    // Groups of <= GS_CAP members are ranked in LDS (group_sort); members of larger groups
    // go through two chained stable radix sorts (key, then dense group number).
    // Text rounds advance h linearly; they pay off while each round resolves most ties
    // (natural-language LCPs).  When a round leaves more than 60 % of its list tied, or large
    // groups dominate, the data is repetitive: rank rounds, logarithmic in the LCP, take over.
    int local_round(bool use_text, bool *bail, const u32 *key_of_suffix = nullptr)
    {
        *bail = false;
        LocalRound r(use_text, key_of_suffix, h, m, !knobs.no_mid_tier);
        PSS_TRY(ctx->slot[S_SCR].reserve(RoundScratch::reserved(m)));
        r.bind(ctx->slot[S_SCR].as<u8>());
        make_keys(r);
        rank_small_groups(r);
        if (!knobs.no_mid_tier) PSS_TRY(middle_tier(r));
        PSS_TRY(count_big(r));
        if (r.nbig == 0) return PSS_OK;
        if (use_text && text_round_gives_up(r.nbig, m, text_rounds, subset)) {
            *bail = true;
            return PSS_OK;
        }
        PSS_TRY(compact_big(r));
        PSS_TRY(periodic_keys(r));
        if (big_route(knobs.big_merge, r.nbig, r.nbig_groups, use_text, r.big_key_bits) == BIG_MERGE) return merge_big(r);
        return chain_big(r);
    }

    void make_keys(LocalRound &r)
    {
        if (r.use_text)
            hipLaunchKernelGGL(text_keys_kernel, dim3(grid), dim3(256), 0, s, V[src], m, text_n, r.h32, codes, b, kt, plus_one,
                               K[src], io.sub_pos);
        else if (r.key_of_suffix)
            hipLaunchKernelGGL(rank_keys_kernel, dim3(grid), dim3(256), 0, s, V[src], m, n, 0u, r.key_of_suffix, K[src]);
        else
            hipLaunchKernelGGL(rank_keys_kernel, dim3(grid), dim3(256), 0, s, V[src], m, n, r.h32, ISA, K[src]);
    }

    void rank_small_groups(LocalRound &r)
    {
        const u32 nblk = r.L.nblk;
        if (r.use_text)
            hipLaunchKernelGGL(group_sort_kernel<false>, dim3(nblk), dim3(256), 0, s, K[src], V[src], G[gcur], m, K[src ^ 1],
                               V[src ^ 1], r.d_big, r.d_blk_big, r.d_blk_heads);
        else if (knobs.count_sort)
            hipLaunchKernelGGL(group_sort_kernel<true>, dim3(nblk), dim3(256), 0, s, K[src], V[src], G[gcur], m, K[src ^ 1],
                               V[src ^ 1], r.d_big, r.d_blk_big, r.d_blk_heads);
        else
            hipLaunchKernelGGL(group_msort32_kernel, dim3(nblk), dim3(GM_BLOCK), 0, s, K[src], V[src], G[gcur], m, K[src ^ 1],
                               V[src ^ 1], r.d_big, r.d_blk_big, r.d_blk_heads);
    }

    // groups of up to MID_CAP members: one workgroup each, in LDS (no host round trip: the list and its
    // length stay on the device, the workgroups persist and walk over it)
    int middle_tier(LocalRound &r)
    {
        u8 *scr = ctx->slot[S_SCR].as<u8>();
        MidGroup *d_mid = region<MidGroup>(scr, r.L.mid), *d_mid_fail = region<MidGroup>(scr, r.L.mid_fail);
        u32 *d_mid_count = region<u32>(scr, r.L.mid_count);
        PSS_HIP(hipMemsetAsync(d_mid_count, 0, 8, s));
        hipLaunchKernelGGL(mid_collect_kernel, dim3(grid), dim3(256), 0, s, r.d_big, G[gcur], m, d_mid, d_mid_count);
        hipLaunchKernelGGL(mid_sort_kernel, dim3((u32)ctx->num_cus * 4), dim3(MID_BLOCK), 0, s, K[src], V[src], d_mid,
                           (const u32 *)d_mid_count, r.use_text ? kt * b : rbits, K[src ^ 1], V[src ^ 1], r.d_big, r.d_blk_big,
                           r.d_blk_heads, knobs.no_mid_merge ? (MidGroup *)nullptr : d_mid_fail, d_mid_count + 1);
        if (!knobs.no_mid_merge)
            hipLaunchKernelGGL(mid_msort_kernel, dim3((u32)ctx->num_cus * 3), dim3(MID_BLOCK), 0, s, K[src], V[src], d_mid_fail,
                               (const u32 *)(d_mid_count + 1), K[src ^ 1], V[src ^ 1], r.d_big, r.d_blk_big, r.d_blk_heads);
        return PSS_OK;
    }

    // The first wait: how many members the large groups have.
    int count_big(LocalRound &r)
    {
        PSS_TRY(device_excl_scan(ctx, InU32{r.d_blk_big}, r.L.nblk, r.d_partial, r.d_total, r.d_off_big));
        PSS_HIP(hipMemcpyAsync(h_small, r.d_total, 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        r.nbig = h_small[0];
        if (knobs.timing)
            fprintf(stderr, "[pss] %s round: h=%llu m=%u large-group members=%u (%.1f%%)\n", r.use_text ? "text" : "rank",
                    (unsigned long long)h, m, r.nbig, 100.0 * r.nbig / m);
        last_big_frac = (double)r.nbig / (double)m;
        return PSS_OK;
    }

    // The second wait: the members compacted, and how many groups they form.
    int compact_big(LocalRound &r)
    {
        const BigScratch B(r.nbig);
        PSS_TRY(ctx->slot[S_BIG].reserve(BigScratch::reserved(r.nbig)));
        u8 *bscr = ctx->slot[S_BIG].as<u8>();
        r.d_bt = region<u32>(bscr, B.bt);
        r.d_bgid = region<u32>(bscr, B.bgid);
        for (int i = 0; i < 2; ++i) {
            r.BK[i] = region<u64>(bscr, B.BK[i]);
            r.BV[i] = region<u32>(bscr, B.BV[i]);
        }
        PSS_TRY(device_excl_scan(ctx, InU32{r.d_blk_heads}, r.L.nblk, r.d_partial, r.d_total, r.d_off_heads));
        PSS_HIP(hipMemcpyAsync(h_small, r.d_total, 8, hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(big_compact_kernel, dim3(r.L.nblk), dim3(256), 0, s, r.d_big, G[gcur], K[src], m, r.d_off_big,
                           r.d_off_heads, r.d_bt, r.BK[0], r.d_bgid);
        PSS_HIP(hipStreamSynchronize(s));
        r.nbig_groups = h_small[0];
        r.gid_bits = index_bits(r.nbig_groups);
        r.big_key_bits = r.use_text ? kt * b : rbits;
        return PSS_OK;
    }

    // periodic runs among the large groups: their members get the key that orders them at once (per_*_kernel)
    int periodic_keys(LocalRound &r)
    {
        const u32 nbig = r.nbig, nbig_groups = r.nbig_groups;
        last_per = false;
        const bool per_syms = (subset || rank_only) ? Xsym != nullptr : codes != nullptr;
        if (per_wait_h > h && nbig >= 2) last_per = true;      // (chains seen, their period still ahead of the depth)
        if (r.use_text || r.key_of_suffix || knobs.no_periodic || !per_syms || nbig < 2 || h >= (1ull << 31) || h < per_wait_h) return PSS_OK;
        const int idx_bits = index_bits(n);
        const PerScratch Y(nbig, nbig_groups);
        if (ctx->slot[S_PER].reserve(Y.reserved()) != PSS_OK) {
            (void)hipGetLastError();
            set_error("%s", "");
            return PSS_OK;
        }
        u8 *pb = ctx->slot[S_PER].as<u8>();
        u64 *PK[2] = {region<u64>(pb, Y.PK0), r.BK[1]};
        u32 *PV[2] = {region<u32>(pb, Y.PV0), r.BV[1]};
        u32 *d_step = region<u32>(pb, Y.step), *d_flag = region<u32>(pb, Y.flag);
        u64 *d_c = region<u64>(pb, Y.c);
        u32 *d_epos = region<u32>(pb, Y.epos), *d_eell = region<u32>(pb, Y.eell);
        u64 *d_etail = region<u64>(pb, Y.etail);
        u32 *d_pmin = region<u32>(pb, Y.pmin);
        u32 *d_gsize = region<u32>(pb, Y.gsize), *d_links = region<u32>(pb, Y.links), *d_bad = region<u32>(pb, Y.bad);
        u32 *d_pg = region<u32>(pb, Y.pg), *d_out = region<u32>(pb, Y.out);
        const u32 pgrid = std::min<u32>((nbig + 255) / 256, (u32)ctx->num_cus * 16);
        const u32 wgrid = std::min<u32>((nbig + 255) / 256, (u32)ctx->num_cus * 4);      // (waves that walk contiguous pieces)
        PSS_HIP(hipMemsetAsync(d_pmin, 0xff, Y.g4, s));
        PSS_HIP(hipMemsetAsync(pb + Y.zeroed, 0, Y.zeroed_bytes, s));      // gsize, links, bad, pg, out
        PSS_HIP(hipMemsetAsync(d_out + 2, 0xff, 4, s));
        hipLaunchKernelGGL(per_pack_kernel, dim3(pgrid), dim3(256), 0, s, r.d_bt, r.d_bgid, V[src], nbig, idx_bits, PK[0], PV[0]);
        int dp = 0;
        SortStats sp;
        PSS_TRY(radix_sort_pairs(ctx, PK, PV, nbig, r.gid_bits + idx_bits, 0xffffffffu, nullptr, 0, io.work, &dp, false, &sp));
        hipLaunchKernelGGL(per_steps_kernel, dim3(wgrid), dim3(256), 0, s, PK[dp], nbig, idx_bits, r.h32, d_step, d_pmin, d_gsize);
        hipLaunchKernelGGL(per_check_kernel, dim3(wgrid), dim3(256), 0, s, PK[dp], d_step, nbig, idx_bits, r.h32, d_pmin,
                           d_links, d_bad, d_out);
        hipLaunchKernelGGL(per_decide_kernel, dim3((nbig_groups + 255) / 256), dim3(256), 0, s, d_pmin, d_gsize, d_links,
                           d_bad, nbig_groups, d_pg, d_out);
        PSS_HIP(hipMemcpyAsync(h_small, d_out, 12, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        const u32 per_members = h_small[0], arith = h_small[1];
        per_wait_h = per_wait(per_members, arith, h_small[2], nbig);
        if (knobs.timing)
            fprintf(stderr, "[pss] rank round: h=%llu large-group members=%u in periodic groups=%u, equal steps=%u\n",
                    (unsigned long long)h, nbig, per_members, arith);
        last_per = per_seen(per_members, arith, nbig);
        if (per_members) {
            const PerSyms y{(subset || rank_only) ? Xsym : nullptr, (subset || rank_only) ? nullptr : codes, n};
            hipLaunchKernelGGL(per_flag_kernel, dim3(pgrid), dim3(256), 0, s, PK[dp], d_step, nbig, idx_bits, d_pg, d_flag);
            PSS_TRY(device_excl_scan(ctx, InU32{d_flag}, nbig, r.d_partial, r.d_total, d_c));
            hipLaunchKernelGGL(per_ends_kernel, dim3(pgrid), dim3(256), 0, s, PK[dp], d_flag, d_c, nbig, idx_bits, d_pg, r.h32,
                               y, ISA, d_epos, d_eell, d_etail);
            hipLaunchKernelGGL(per_keys_kernel, dim3(pgrid), dim3(256), 0, s, PK[dp], PV[dp], d_c, nbig, idx_bits, d_pg, d_epos,
                               d_eell, d_etail, r.d_bt, r.BK[0], K[src]);
            r.big_key_bits = 64;
            st.periodic_rounds += 1;
            st.periodic_members += per_members;
        }
        st.round_passes += (u32)sp.launches;
        return PSS_OK;
    }

    // segmented merge sort of the large groups (bg_*_kernel): tiles in LDS, then merge passes inside every group
    int merge_big(LocalRound &r)
    {
        const u32 nbig = r.nbig, nbig_groups = r.nbig_groups;
        const BigTiles T(nbig, nbig_groups);
        const u32 bound = T.bound;
        PSS_TRY(ctx->slot[S_BGT].reserve(T.reserved()));
        u8 *tb = ctx->slot[S_BGT].as<u8>();
        u32 *d_gstart = region<u32>(tb, T.gstart);
        u64 *d_toff = region<u64>(tb, T.toff);
        BigTile *d_tiles = region<BigTile>(tb, T.tiles);
        const u32 eg = std::min<u32>((nbig + 255) / 256, (u32)ctx->num_cus * 16);
        hipLaunchKernelGGL(bg_gstart_kernel, dim3(eg), dim3(256), 0, s, r.d_bgid, nbig, nbig_groups, d_gstart);
        PSS_TRY(device_excl_scan(ctx, InTileCount{d_gstart}, nbig_groups, r.d_partial, r.d_total, d_toff));
        PSS_HIP(hipMemsetAsync(d_tiles, 0, (size_t)bound * sizeof(BigTile), s));
        hipLaunchKernelGGL(bg_tiles_kernel, dim3(std::min<u32>((nbig_groups + 3) / 4, (u32)ctx->num_cus * 8)), dim3(256), 0, s, d_gstart,
                           d_toff, nbig_groups, d_tiles);
        hipLaunchKernelGGL(bg_gather_kernel, dim3(eg), dim3(256), 0, s, r.d_bt, V[src], nbig, r.BV[0]);
        const u32 wg = std::min<u32>(bound, (u32)ctx->num_cus * 2);
        hipLaunchKernelGGL(bg_tile_sort_kernel, dim3(wg), dim3(BG_BLOCK), 0, s, r.BK[0], r.BV[0], d_tiles, bound, r.BK[1], r.BV[1]);
        int from = 1;
        for (u64 L = BG_TILE; L < (u64)nbig; L <<= 1) {
            hipLaunchKernelGGL(bg_merge_kernel, dim3(wg), dim3(BG_BLOCK), 0, s, r.BK[from], r.BV[from], r.BK[from ^ 1], r.BV[from ^ 1], d_tiles,
                               bound, (u32)L);
            from ^= 1;
        }
        hipLaunchKernelGGL(bg_writeback_kernel, dim3(std::min<u32>(bound, (u32)ctx->num_cus * 8)), dim3(256), 0, s, r.BK[0], r.BV[0], r.BK[1],
                           r.BV[1], d_tiles, bound, r.d_bt, K[src ^ 1], V[src ^ 1]);
        st.big_elems += nbig;
        return PSS_OK;
    }

    // two chained stable radix sorts: by key, then by dense group number
    int chain_big(LocalRound &r)
    {
        const u32 nbig = r.nbig;
        hipLaunchKernelGGL(iota_kernel, dim3((nbig + 255) / 256), dim3(256), 0, s, r.BV[0], nbig);
        SortStats both, s2;
        int d1 = 0, d2 = 0;
        PSS_TRY(radix_sort_pairs(ctx, r.BK, r.BV, nbig, r.big_key_bits, 0xffffffffu, nullptr, 0, io.work, &d1, io.profile, &both));
        hipLaunchKernelGGL(gather_gid_kernel, dim3((nbig + 255) / 256), dim3(256), 0, s, r.BV[d1], r.d_bgid, nbig,
                           nbig <= 4096u, r.BK[d1]);
        if (r.nbig_groups > 1)
            // (unique keys carry v in their low word: the one-workgroup sort then compares all 64 bits)
            PSS_TRY(radix_sort_pairs(ctx, r.BK, r.BV, nbig, nbig <= 4096u ? 64 : r.gid_bits, 0xffffffffu, nullptr, d1, io.work, &d2,
                                     io.profile, &s2));
        else d2 = d1;
        hipLaunchKernelGGL(big_writeback_kernel, dim3((nbig + 255) / 256), dim3(256), 0, s, r.BV[d2], r.d_bt, K[src],
                           V[src], nbig, K[src ^ 1], V[src ^ 1]);
        both += s2;
        st.round_passes += (u32)both.launches;
        ss += both;
        st.big_elems += nbig;
        return PSS_OK;
    }

    // ------------------------------------------------------ text rounds and the anchor round in their place --
    bool anchors_on() const { return !subset && knobs.anchor != 0 && (knobs.anchor == 1 || n >= (1u << 20)); }
    bool side_on() const { return knobs.side != 0 && !rank_only && (knobs.side == 1 || n >= (1u << 24)) && io.level == 0; }

    int text_stage(Took *took)
    {
        bool skip_text = false, side_wanted = false;
        PSS_TRY(probe(&skip_text, &side_wanted));
        PSS_TRY(maybe_start_side(skip_text, side_wanted));
        bool bail = true;
        PSS_TRY(text_round(skip_text, &bail));
        if (bail && !anchored && anchors_on()) {
            // Ties that outlive the text rounds are repeats: one round keyed by the ranks of the anchors (anchor_impl.h)
            // instead of log2(length of the repeat) rank rounds over the whole text.  The key array takes the place
            // of the inverse suffix array, which this path never builds.
            const u32 *akey = nullptr;
            PSS_TRY(take_side(&akey));
            if (!akey) {
                bool ok = false;
                PSS_TRY(anchor_rank_keys(ctx, knobs, io, h, nullptr, nullptr, ISA, st, &ok));
                if (ok) akey = ISA;
            }
            if (akey) {
                st.anchor_active = m;
                return anchor_round(akey, took);
            }
        }
        if (!bail) return took_round(Took::text, took);
        // ties outlived the text rounds: build the inverse suffix array once, continue with rank rounds
        hipLaunchKernelGGL(isa_from_sa_kernel, dim3(grid_all), dim3(256), 0, s, SA, n, ISA);
        hipLaunchKernelGGL(isa_active_kernel, dim3(grid), dim3(256), 0, s, V[src], G[gcur], m, ISA);
        mode = M_DENSE;
        if (subset) {
            h = 1;               // from here on the elements are the symbols of an integer string
            PSS_TRY(snapshot_symbols());
        }
        return PSS_OK;
    }

    // are these ties repeats (see probe_repeats_kernel)?  Then no text round will resolve them.
    int probe(bool *skip_text, bool *side_wanted)
    {
        const bool probe_skips = h >= (u64)knobs.anchor_min_omega + 3;       // deep enough for the anchor round to run at once
        if (!(anchors_on() && !anchored && text_rounds == 0 && !knobs.no_probe && m >= 4096 && (u64)m * 16 >= (u64)n && (probe_skips || side_on())))
            return PSS_OK;
        u32 *d_probe = io.sm.counters + 48;
        PSS_HIP(hipMemsetAsync(d_probe, 0, 8, s));
        const u32 samples = 8192;
        hipLaunchKernelGGL(probe_repeats_kernel, dim3(samples / 256), dim3(256), 0, s, V[src], G[gcur], m, samples, n,
                           (u32)std::min<u64>(h, 0xffffffffull), codes, d_probe);
        PSS_HIP(hipMemcpyAsync(h_small, d_probe, 8, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        st.probe_pairs = h_small[0];
        st.probe_same = h_small[1];
        *skip_text = probe_skips_text(probe_skips, h_small[0], h_small[1], knobs.probe_skip_pct);
        *side_wanted = probe_wants_side(side_on(), *skip_text, h_small[0], h_small[1], knobs.side_pct);
        if (knobs.timing) fprintf(stderr, "[pss] probe: %u of %u sampled pairs share 48 more symbols%s\n", h_small[1], h_small[0], *skip_text ? ": no text rounds" : (*side_wanted ? ": anchors beside the text round" : ""));
        return PSS_OK;
    }

    int maybe_start_side(bool skip_text, bool side_wanted)
    {
        if (knobs.side == 1 && side_on() && anchors_on() && !anchored && text_rounds == 0 && !skip_text) side_wanted = true;
        if (side_wanted && !side.started && text_rounds < knobs.text_rounds_max)
            // the depth the coming text round will reach decides the window; the anchors' sort starts now, on the side
            PSS_TRY(side_start(ctx, knobs, side, n, codes, b, plus_one, h + (u64)kt, nullptr));
        return PSS_OK;
    }

    // *bail stays true where no text round runs, or the one that ran gave up.
    int text_round(bool skip_text, bool *bail)
    {
        const bool text_progress = text_rounds == 0 || (u64)m * 10 <= (u64)m_text_prev * 6;
        if (anchored) {
            // cannot happen: the anchor round leaves no ties.  Counted (tests assert zero) and resolved by rank rounds.
            st.anchor_left += m;
        } else if (skip_text) {
        } else if (subset) {
            if (h < io.stop_text_h) PSS_TRY(local_round(true, bail));
        } else if (text_rounds < knobs.text_rounds_max && text_progress) {
            m_text_prev = m;
            PSS_TRY(local_round(true, bail));
        }
        return PSS_OK;
    }

    // The side line, if one was started: joined, and its keys adopted (*akey) where they are valid for this depth.
    int take_side(const u32 **akey)
    {
        if (!side.started) return PSS_OK;
        side.join();
        if (side.rc == PSS_ENOMEM) {
            // no room for the side line's buffers is not an error of the build (side_start says so about its own
            // reservations; the same holds for what the helper context grows later): give its slots back and let
            // the anchors wait their turn on the main line
            if (ctx->helper)
                for (auto &sl : ctx->helper->slot) sl.release();
            (void)hipGetLastError();
            set_error("%s", "");
            side.ok = false;
        } else if (side.rc != PSS_OK) {
            set_error("%s", side.err.c_str());
            return side.rc;
        }
        if (!(side.ok && h >= side.h_eff)) {
            st.anchor_side = 2;      // thrown away: the text round gave up before it reached the window's depth, or the round declined
            return PSS_OK;
        }
        // sorted beside the text round: its keys are valid for every depth from h_eff on
        const pss_sa_stats &t = side.st;
        st.anchor = 1;
        st.anchor_count = t.anchor_count;
        st.anchor_omega = t.anchor_omega;
        st.anchor_w = t.anchor_w;
        st.anchor_ms += t.anchor_ms;
        st.anchor_depth = h;
        st.anchor_text_rounds += t.anchor_text_rounds;
        st.anchor_rounds += t.anchor_rounds;
        st.anchor_sum_active += t.anchor_sum_active;
        st.anchor_left += t.anchor_left;
        st.periodic_rounds += t.periodic_rounds;
        st.periodic_members += t.periodic_members;
        st.anchor_levels = std::max<uint64_t>(st.anchor_levels, t.anchor_levels);
        st.anchor_side = 1;
        *akey = side.akey;
        return PSS_OK;
    }

    // One round keyed by the ranks of the anchors: nothing is left tied.
    int anchor_round(const u32 *akey, Took *took)
    {
        bool b2 = false;
        PSS_TRY(local_round(false, &b2, akey));
        anchored = true;
        return took_round(Took::anchor, took);
    }

    // a level up: minimizers of this string of symbols, named by the ranks the rounds have reached
    int level_up(Took *took)
    {
        if (!(mode == M_DENSE && X0 && !anchored && h >= 32 && (u64)m * 16 >= (u64)n && m >= (knobs.anchor == 1 ? 64u : (1u << 19)))) return PSS_OK;
        bool ok = false;
        PSS_TRY(anchor_rank_keys(ctx, knobs, io, h, X0, ISA, ISA, st, &ok));
        if (ok) return anchor_round(ISA, took);
        X0 = nullptr;            // declined: plain rounds to the end
        return PSS_OK;
    }

    // Rank rounds: group-local unless large groups dominate (goes_global).
    int rank_round(Took *took)
    {
        if (mode == M_DENSE && m <= global_above) global_above = 0;
        if (!(mode == M_DENSE && global_above == 0)) return PSS_OK;
        bool bail = false;
        PSS_TRY(local_round(false, &bail));
        global_above = goes_global(last_big_frac, last_per, m);
        return took_round(Took::rank, took);
    }

    // ------------- global doubling round: sparse (hash table + key search) or dense (ISA) --
    int global_round()
    {
        keyed_grp = true;
        if (mode == M_SPARSE && round == 0) {
            // hash table over the initially-active suffixes, in the (unused) ISA buffer
            u32 cap = 1024;
            while (cap < 4u * m) cap <<= 1;
            ra.ht_mask = cap - 1;
            PSS_HIP(hipMemsetAsync(ra.ht, 0, (size_t)cap * 8, s));
            hipLaunchKernelGGL(ht_insert_kernel, dim3(grid), dim3(256), 0, s, ra.ht, ra.ht_mask, V[src], G[gcur], m);
            // small key buffers carved out of the free big key buffer
            SK[0] = K[k0buf ^ 1];
            SK[1] = K[k0buf ^ 1] + (size_t)m;
            Kr = SK;
        }
        h_small[0] = 0; h_small[1] = 0; h_small[2] = 0xffffffffu; h_small[3] = 0xffffffffu;
        PSS_HIP(hipMemcpyAsync(io.sm.red, h_small, 16, hipMemcpyHostToDevice, s));
        KeyArgs ka;
        ka.idx = V[src];
        ka.grp = G[gcur];
        ka.ISA = ISA;
        ka.ht = ra.ht;
        ka.ht_mask = ra.ht_mask;
        ka.sa = SA;
        ka.codes = codes;
        ka.code_bits = b;
        ka.key_chars = io.key_chars;
        ka.plus_one = plus_one;
        ka.m = m;
        ka.n = n;
        ka.h = (u32)std::min<u64>(h, 0xffffffffull);
        ka.rank_bits = rbits;
        ka.keys = Kr[src];
        ka.red = io.sm.red;
        const u32 grid_keys = std::max(1u, std::min(grid, (m + 2047u) / 2048u));   // >= 8 keys per thread: fewer atomics on the two words
        if (mode == M_SPARSE) hipLaunchKernelGGL(build_keys_kernel<true>, dim3(grid), dim3(256), 0, s, ka);   // latency-bound key searches: every wave helps
        else hipLaunchKernelGGL(build_keys_kernel<false>, dim3(grid_keys), dim3(256), 0, s, ka);
        PSS_HIP(hipMemcpyAsync(h_small, io.sm.red, 16, hipMemcpyDeviceToHost, s));
        PSS_HIP(hipStreamSynchronize(s));
        const u64 vor = (u64)h_small[0] | ((u64)h_small[1] << 32);
        const u64 vand = (u64)h_small[2] | ((u64)h_small[3] << 32);
        const int key_bits = 2 * rbits;
        SortStats rs;
        PSS_TRY(radix_sort_pairs(ctx, Kr, V, m, key_bits, varying_digits(vor, vand, key_bits), nullptr, src, io.work, &cur, io.profile, &rs));
        st.rounds += 1;
        st.round_passes += (u32)rs.launches;
        st.sum_active += m;
        ss += rs;
        h *= 2;
        return PSS_OK;
    }
};
