// seq_class_impl.h -- the wildcard search whose segments hold BYTE CLASSES (`?`, `[set]`, `[!set]`) beside literal bytes
// (include/pss.h, pss_reader_search_seqc_batch).  Part of search.hip: included there behind
// sequence_impl.h, whose walk it repeats; not a header for anybody else.
//
// Between two `*` such a pattern is still a piece of FIXED LENGTH, so the leftmost-greedy walk of seq_verify_kernel is
// complete as it stands: its argument never looks at how a byte of the entry is compared with a position of the segment.
// What changes is how a segment is FOUND.  A segment with a literal run has a CORE (its longest one, the leftmost on a
// tie): the cores are the terms of the batch, so the interval search, the driver choice and the candidate kernels ran over
// them unchanged, and here the core is what entry_scan looks for; every place it is found at is then tested against the
// segment's other positions.  A segment without a core is tested start position by start position.

// One class batch's segments as the verify kernel reads them (SearchRequest's class block, on the device).
struct SeqClass {
    const u8 *bytes;        // one byte per position: the literal (folded under Fold), 0 at a class position; 32 zero bytes behind
    const u8 *plane;        // one byte per position: 0 = literal, else the 1-based index of the position's set
    const u64 *off;         // nsegs + 1: the segments inside bytes / plane
    const u64 *goff;        // ngroups + 1: the groups' segments
    const u32 *core;        // two per segment: core offset and core length; length 0: no core, offset 1 iff all positions are `?`
    const u32 *sets;        // eight words per set: bit b = word b >> 5, bit b & 31
};

__device__ __forceinline__ bool class_holds(const u32 *sets, u32 k, u32 b) { return (sets[(k - 1) * 8 + (b >> 5)] >> (b & 31)) & 1u; }

// Does position i of the segment (sb / sp: its bytes and plane) accept the byte b of the entry?  Under Fold a literal is
// folded already and the sets are closed under the fold, so b is folded for the literal alone.
template <bool Fold>
__device__ __forceinline__ bool position_fits(const SeqClass &sc, const u8 *sb, const u8 *sp, u32 i, u32 b)
{
    const u32 k = sp[i];
    if (k) return class_holds(sc.sets, k, b);
    if (Fold && b - 'A' < 26u) b |= 0x20u;
    return b == sb[i];
}

// Do the positions of the segment outside its core [co, co + cl) accept text[p, p + L)?  The caller knows p + L <= lim, so
// nothing behind lim is read.  Lane gl takes the positions gl, gl + TG, ...; the lanes agree by one ballot, which they
// reach together: the per-lane loop closes in front of it.
template <bool Fold>
__device__ __forceinline__ bool classes_fit(const ChunkDesc &ch, const SeqClass &sc, const u8 *sb, const u8 *sp, u32 L, u32 co, u32 cl,
                                            u32 p, u32 gl, u32 gbase)
{
    bool miss = false;
    for (u32 i = gl; i < L && !miss; i += TG)
        if (i - co >= cl) miss = !position_fits<Fold>(sc, sb, sp, i, ch.text[p + i]);     // (i < co wraps: outside the core too)
    return ((u32)(__ballot(miss) >> gbase) & ((1u << TG) - 1u)) == 0;
}

// The LEFTMOST p in from .. lim - L at which segment j (L positions) fits text[p, p + L), or kNone; for the TG lanes of one
// group together, every lane returns the group's answer.  lim <= n and lim is at most the entry's true end, so a window
// [p, p + L) that is read lies inside the entry: a `?` or a negated set never sees the closing newline, and a set that
// holds 0x00 never the zero padding behind the chunk.
//   A segment with a core: entry_scan<Fold, true> for the core over the start positions from + co .. lim - L + co -- the
//   places at which the WHOLE segment still lies in [from, lim): a core that stands nearer to `from` than co, or nearer to
//   lim than L - co, is never reported, so p < from and p + L > lim are rejected before anything is read.  At a finding q
//   the other positions are tested at p = q - co; on a miss the scan goes on from q + 1, so overlapping occurrences of the
//   core are all seen.  Every trip moves q forward by at least one: at most lim - from trips, each one scan step and
//   L / TG byte tests per lane beyond what entry_scan itself walks.
//   A segment without a core: all `?` fits at `from` whenever it fits at all; else lane gl tests the start positions
//   base + gl, one position of the segment after the other, and the lowest lane that found one holds the leftmost (the
//   entry_scan idiom): (lim - from) / TG trips of at most L byte tests per lane.
// INVARIANT (the ballots here and in entry_scan): every branch between the calling kernel's loop entry and a ballot depends
// on group-wide values only -- the segment (L, co, cl), from, lim, q and base, which follow from entry_scan's answers and
// from ballots read through the group's own bits -- never on gl; the per-lane loops and the `p <= last` test close in front
// of the ballot behind them.
template <bool Fold>
__device__ __forceinline__ u32 seg_find(const ChunkDesc &ch, const SeqClass &sc, u32 j, u32 from, u32 lim, u32 gl, u32 gbase)
{
    const u64 o = sc.off[j];
    const u32 L = (u32)(sc.off[j + 1] - o);
    if (from > lim || L > lim - from) return kNone;
    const u8 *sb = sc.bytes + o, *sp = sc.plane + o;
    const u32 co = sc.core[2 * j], cl = sc.core[2 * j + 1];
    if (cl) {
        const u32 qlast = lim - L + co;
        u32 q = from + co;
        while (q <= qlast) {
            q = entry_scan<Fold, true>(ch, q, qlast, sb + co, cl, gl, gbase);
            if (q == kNone) return kNone;
            if (cl == L || classes_fit<Fold>(ch, sc, sb, sp, L, co, cl, q - co, gl, gbase)) return q - co;
            ++q;
        }
        return kNone;
    }
    if (co) return from;                                         // a run of `?`: any L bytes of the entry
    const u32 last = lim - L;
    for (u64 base = from; base <= last; base += TG) {            // (the same trips for every lane of the group)
        const u64 p = base + gl;
        bool fits = p <= last;
        for (u32 i = 0; i < L && fits; ++i) fits = class_holds(sc.sets, sp[i], ch.text[(u32)p + i]);
        const u32 who = (u32)(__ballot(fits) >> gbase) & ((1u << TG) - 1u);
        if (who) return (u32)base + (u32)__builtin_ctz(who);
    }
    return kNone;
}

// seq_verify_kernel for a class batch: the same candidates (one per entry that holds the pair's driving core), the same
// walk -- END pins the last segment to the entry's end, START the first to its start, the rest left to right, each at its
// leftmost place behind the one before it -- and the same shape: TG = 8 lanes per candidate, 32 candidates per 256-thread
// workgroup, grid-stride.  A segment's length is its position count.  The driving core's segment is placed like any other.
// It writes len[t] = kSkip alone, from gl == 0.  No LDS, no scratch.
template <bool Fold>
__global__ __launch_bounds__(256) void seqc_verify_kernel(const ChunkDesc *chunks, u32 nc, SeqClass sc, const u8 *anchors, u64 ngq,
                                                            const u64 *hit_off, u64 H, const u32 *start, u32 *len)
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
        u32 j0 = (u32)sc.goff[g], j1 = (u32)sc.goff[g + 1];      // the segments still to place: [j0, j1)
        const u8 anch = anchors[g];
        u32 from = s, lim = end;
        bool ok = true;
        if ((anch & 3u) == 3u && j1 - j0 == 1) {                 // one segment, both anchors: the entry is as long and fits
            const u32 pl = (u32)(sc.off[j0 + 1] - sc.off[j0]);
            ok = pl == end - s && seg_find<Fold>(ch, sc, j0, s, end, gl, gbase) != kNone;
            j0 = j1;
        }
        if (ok && (anch & 2u) && j0 < j1) {                      // END: the last segment sits at the entry's end
            --j1;
            const u32 pl = (u32)(sc.off[j1 + 1] - sc.off[j1]);
            ok = pl <= end - s && seg_find<Fold>(ch, sc, j1, end - pl, end, gl, gbase) != kNone;
            if (ok) lim = end - pl;
        }
        if (ok && (anch & 1u) && j0 < j1) {                      // START: the first segment sits at the entry's start
            const u32 pl = (u32)(sc.off[j0 + 1] - sc.off[j0]);
            ok = pl <= lim - s && seg_find<Fold>(ch, sc, j0, s, s + pl, gl, gbase) != kNone;       // (lim >= s)
            from = s + pl;                                       // (ok: from <= lim, the two anchored segments do not overlap)
            ++j0;
        }
        for (u32 j = j0; j < j1 && ok; ++j) {
            const u32 p = seg_find<Fold>(ch, sc, j, from, lim, gl, gbase);
            ok = p != kNone;
            from = p + (u32)(sc.off[j + 1] - sc.off[j]);
        }
        if (!ok && gl == 0) len[t] = kSkip;
    }
}
