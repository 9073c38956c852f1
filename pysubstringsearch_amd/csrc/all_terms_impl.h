// all_terms_impl.h -- entries that contain ALL the include terms of a group and NONE of its exclude terms (include/pss.h,
// pss_reader_search_terms_batch).
// Part of search.hip: included there behind the entry helpers (hit_entry, pair_of_hit), entry_scan_impl.h and the
// workspace slots; not a header for anybody else.
//
// A batch of ng groups over nterms terms has TWO pair spaces:
//   term pairs   (term, chunk), nterms x nc: what the interval kernels of search.hip answer, unchanged -- lo and count of
//                every term in every chunk before a single hit is touched;
//   group pairs  (group, chunk), ng x nc: what everything from the first scan on runs over.
// terms_driver_kernel joins them: per group pair it picks the include term with the fewest hits in that chunk (the
// lowest index on a tie) and hands its interval on as the pair's.  A chunk where an include term is absent counts zero
// hits for the pair.  hit_lines_kernel, given the drivers, takes each pair's pattern from them: leftmost-match dedupe and
// entry bounds, one candidate per entry that holds the driver.  terms_verify_kernel then scans each candidate entry
// (entry_scan) once for the group's other terms and marks it kSkip when an include term is missing or an exclude term is
// there; the kept-hit scan, the counts and the two emit kernels of the general pipeline run as always.
// A term that holds a 0x0A occurs in no entry, but its interval need not be empty (it may match across entries): such a
// term is flagged on the host (newline_flags).  As an include term it voids its group, as an exclude term it is ignored.

constexpr u8 kTermExclude = 1;
constexpr u8 kTermVoid = 0x80;                   // the term holds a newline: it occurs in no entry

// One lane per (group, chunk) pair: the driver term of the pair, its interval and its hit count.
// Lo = false: the terms have no interval of their own (the terms of a seeded batch, seed_impl.h: cnt is the sum over a
// term's seed queries), so lo is not read and g_lo not written.
template <bool Lo>
__global__ __launch_bounds__(256) void terms_driver_kernel(u32 nc, const u64 *goff, const u8 *flags, const u32 *lo, const u32 *cnt,
                                                             u64 ngq, u32 *g_drv, u32 *g_lo, u32 *g_cnt)
{
    const u64 gq = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gq >= ngq) return;
    const u32 g = (u32)(gq / nc), c = (u32)(gq % nc);
    const u32 t0 = (u32)goff[g], t1 = (u32)goff[g + 1];
    u32 best = 0, bt = t0;
    bool have = false, dead = false;
    for (u32 t = t0; t < t1 && !dead; ++t) {
        const u8 f = flags[t];
        if (f & kTermExclude) continue;
        if (f & kTermVoid) {
            dead = true;
            break;
        }
        const u32 k = cnt[(u64)t * nc + c];
        if (!have || k < best) {
            best = k;
            bt = t;
            have = true;
        }
    }
    g_drv[gq] = bt;
    if (Lo) g_lo[gq] = have ? lo[(u64)bt * nc + c] : 0u;
    g_cnt[gq] = (have && !dead) ? best : 0u;
}

// Does text[s, end) hold pat?  entry_scan (entry_scan_impl.h) over the start positions s .. end - plen, for the TG lanes
// of one group together.  Fold: under ASCII case folding, pat folded already; end <= n, so a match at the last start
// position end - plen ends inside the chunk, as entry_scan asks.
template <bool Fold>
__device__ __forceinline__ bool entry_holds(const ChunkDesc &ch, u32 s, u32 end, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    return plen <= end - s && entry_scan<Fold, false>(ch, s, end - plen, pat, plen, gl, gbase) != kNone;
}

// TG lanes per hit the dedupe kept (one per candidate entry): the group's other terms inside the entry [start, true
// end).  The true end is the closing newline or n -- not start + len, which is short by one for an unterminated last
// entry.  An exclude term without a hit in the chunk cannot be in the entry and is not looked for.
// Fold: the terms of a case-insensitive group batch (fold_impl.h).  qbytes / qoff are then the FOLDED terms and cnt the
// terms' seed hits per chunk (seed_union_kernel); a term whose seed is absent from the chunk is absent itself, so the
// exclude shortcut holds as it stands.  The group-wide-branch invariant of entry_scan holds for both forms alike: every
// branch of the loop below depends on t, on what is read at t (l, s, e, the pair and through it g, c, drv) and on the
// group's terms (f, cnt, `found` -- entry_scan's answer, the same in every lane of the group), never on gl.
template <bool Fold>
__global__ __launch_bounds__(256) void terms_verify_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                             const u64 *goff, const u8 *flags, const u32 *cnt, const u32 *g_drv,
                                                             u64 ngq, const u64 *hit_off, u64 H, const u32 *start, u32 *len)
{
    const u32 lane = lane_id(), gl = lane & (TG - 1), gbase = lane & ~(TG - 1);
    const u64 step = (u64)gridDim.x * blockDim.x / TG;
    for (u64 t = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / TG; t < H; t += step) {
        const u32 l = len[t];
        if (l == kSkip) continue;
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = (u32)(a / nc), c = (u32)(a % nc);
        const ChunkDesc ch = chunks[c];
        const u32 s = start[t], e = s + l;                       // e <= n - 1: the closing newline, or the last byte
        const u32 end = ch.text[e] == '\n' ? e : ch.n;
        const u32 drv = g_drv[a], t1 = (u32)goff[g + 1];
        bool ok = true;
        for (u32 j = (u32)goff[g]; j < t1 && ok; ++j) {
            const u8 f = flags[j];
            const bool excl = (f & kTermExclude) != 0;
            if (j == drv || (f & kTermVoid)) continue;           // (a void include term left the pair without hits)
            if (excl && cnt[(u64)j * nc + c] == 0) continue;
            const bool found = entry_holds<Fold>(ch, s, end, qbytes + qoff[j], (u32)(qoff[j + 1] - qoff[j]), gl, gbase);
            ok = found != excl;
        }
        if (!ok && gl == 0) len[t] = kSkip;
    }
}
