// sequence_impl.h -- entries that hold the segments of a group IN ORDER and without overlap, optionally anchored at the
// entry's two ends: the wildcard search `s0*s1*..*sk-1` (include/pss.h, pss_reader_search_seq_batch).
// Part of search.hip: included there behind all_terms_impl.h, whose pair spaces, driver choice and candidate kernel it
// shares; not a header for anybody else.
//
// A sequence batch IS an all-terms batch up to the verify step: the interval search answers every (segment, chunk) pair,
// terms_driver_kernel picks the rarest segment of every (group, chunk) pair (every segment is an include term), and
// hit_lines_kernel over the drivers yields one candidate per entry that holds the driver.  seq_verify_kernel then walks
// each candidate entry once, left to right: it needs WHERE a segment sits, not whether, and entry_scan
// (entry_scan_impl.h) answers with the leftmost position.  The driver segment is matched like any other: its position
// matters.
// A segment that holds a 0x0A occurs in no entry and voids its group (kTermVoid, from newline_flags): the pair counts no
// hit.

// The LEFTMOST occurrence of pat that lies inside text[from, lim), or kNone: entry_scan over the start positions
// from .. lim - plen, for the TG lanes of one group together.  A range of one start position (lim == from + plen) is the
// anchored test: "pat sits exactly at from".  Fold: under ASCII case folding, pat folded already; lim <= n, so a match at
// the last start position lim - plen ends inside the chunk, as entry_scan asks.
template <bool Fold>
__device__ __forceinline__ u32 entry_find(const ChunkDesc &ch, u32 from, u32 lim, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    if (from > lim || plen > lim - from) return kNone;
    return entry_scan<Fold, true>(ch, from, lim - plen, pat, plen, gl, gbase);
}

// TG lanes per hit the dedupe kept (one per candidate entry): the group's segments inside the entry [start, true end),
// in order.  The true end is the closing newline or n -- not start + len, which is short by one for an unterminated last
// entry.  An END anchor pins the last segment to the entry's end and a START anchor the first to its start; what is left
// is walked left to right, each segment at its LEFTMOST occurrence behind the one before it.  Leftmost-greedy is complete
// for patterns whose only wildcard is `*`: if any placement p_0 < p_1 < .. exists, moving p_0 to the leftmost occurrence
// of s_0 keeps every later constraint (p_1 >= p_0 + |s_0| only gets looser), and so on by induction -- no backtracking.
// The same shape as terms_verify_kernel, for the same reasons: TG = 8 lanes per candidate (64 bytes of entry per step),
// 32 candidates per 256-thread workgroup, grid-stride.
// Fold: the patterns of a case-insensitive group batch (fold_impl.h); qbytes / qoff are then the FOLDED segments, and
// every comparison below is under fold.  Leftmost-greedy stays complete: the argument above never looks at how two
// bytes are compared.  The group-wide-branch invariant of entry_scan holds for both forms alike: every branch below
// depends on t, on what is read at t, on the group's segments and anchor byte and on entry_find's answers, which every
// lane of the group holds alike -- never on gl.
template <bool Fold>
__global__ __launch_bounds__(256) void seq_verify_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                           const u64 *goff, const u8 *anchors, u64 ngq, const u64 *hit_off, u64 H,
                                                           const u32 *start, u32 *len)
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
        u32 j0 = (u32)goff[g], j1 = (u32)goff[g + 1];            // the segments still to place: [j0, j1)
        const u8 anch = anchors[g];
        u32 from = s, lim = end;
        bool ok = true;
        if ((anch & 3u) == 3u && j1 - j0 == 1) {                 // one segment, both anchors: the entry equals it
            const u32 pl = (u32)(qoff[j0 + 1] - qoff[j0]);
            ok = pl == end - s && entry_find<Fold>(ch, s, end, qbytes + qoff[j0], pl, gl, gbase) != kNone;
            j0 = j1;
        }
        if (ok && (anch & 2u) && j0 < j1) {                      // END: the last segment sits at the entry's end
            --j1;
            const u32 pl = (u32)(qoff[j1 + 1] - qoff[j1]);
            ok = pl <= end - s && entry_find<Fold>(ch, end - pl, end, qbytes + qoff[j1], pl, gl, gbase) != kNone;
            if (ok) lim = end - pl;
        }
        if (ok && (anch & 1u) && j0 < j1) {                      // START: the first segment sits at the entry's start
            const u32 pl = (u32)(qoff[j0 + 1] - qoff[j0]);
            ok = pl <= lim - s && entry_find<Fold>(ch, s, s + pl, qbytes + qoff[j0], pl, gl, gbase) != kNone;     // (lim >= s)
            from = s + pl;                                       // (ok: from <= lim, the two anchored segments do not overlap)
            ++j0;
        }
        for (u32 j = j0; j < j1 && ok; ++j) {
            const u32 pl = (u32)(qoff[j + 1] - qoff[j]);
            const u32 p = entry_find<Fold>(ch, from, lim, qbytes + qoff[j], pl, gl, gbase);
            ok = p != kNone;
            from = p + pl;
        }
        if (!ok && gl == 0) len[t] = kSkip;
    }
}
