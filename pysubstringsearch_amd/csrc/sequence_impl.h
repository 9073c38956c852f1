// sequence_impl.h -- entries that hold the segments of a group IN ORDER and without overlap, optionally anchored at the
// entry's two ends: the wildcard search `s0*s1*..*sk-1` (include/pss.h, pss_reader_search_seq_batch).
// Part of search.hip: included there behind all_terms_impl.h, whose pair spaces, driver choice and candidate kernel it
// shares; not a header for anybody else.
//
// A sequence batch IS an all-terms batch up to the verify step: the interval search answers every (segment, chunk) pair,
// terms_driver_kernel picks the rarest segment of every (group, chunk) pair (every segment is an include term), and
// terms_hits_kernel yields one candidate per entry that holds the driver.  seq_verify_kernel then walks each candidate
// entry once, left to right: it needs WHERE a segment sits, not whether, so it is built on entry_find -- entry_holds
// with a position for an answer.  The driver segment is matched like any other: its position matters.
// A segment that holds a 0x0A occurs in no entry and voids its group (kTermVoid): the pair counts no hit.

constexpr u32 kNone = 0xffffffffu;               // entry_find: no occurrence

// Per-segment flags of a sequence batch (nseg values): no segment excludes.
static void seq_flags(const u8 *qbytes, const u64 *qoff, u32 nseg, u8 *flags)
{
    for (u32 t = 0; t < nseg; ++t) {
        const u64 m = qoff[t + 1] - qoff[t];
        flags[t] = (m && memchr(qbytes + qoff[t], '\n', m)) ? kTermVoid : 0;
    }
}

// The LEFTMOST occurrence of pat that lies inside text[from, lim), or kNone.  Called by the TG lanes of one group together
// (gl = lane inside the group, gbase = the group's first lane); every lane returns the group's answer.  A match starts at
// from .. lim - plen and nowhere else, so it never reaches the newline at the entry's end, the next entry or the zero
// padding behind the chunk.  The scan is entry_holds': per step the group covers 8 * TG start positions, lane gl the 8
// that begin at its own 8-byte word; a lane stops at the LOWEST matching byte of its word (the ctz loop ascends), and
// among the lanes that found one in a step the LOWEST LANE holds the lowest position, since lane gl's positions all lie
// below lane gl + 1's.  Steps ascend too, so the first step with a finding holds the leftmost occurrence.  Loads reach at
// most 23 bytes past a start position (the text is readable 128 bytes past n, a segment 16 past its end; 32 zero bytes
// follow the staged segments).
// A range of one start position (lim == from + plen) is the anchored test: "pat sits exactly at from".
__device__ __forceinline__ u32 entry_find(const ChunkDesc &ch, u32 from, u32 lim, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    if (from > lim || plen > lim - from) return kNone;
    const u32 last = lim - plen;                                 // the last start position
    const u64 first = 0x0101010101010101ull * pat[0];
    const u64 pmask = plen >= 8 ? ~0ull : (1ull << (8 * plen)) - 1ull;
    const u64 pk = load_u64_unaligned(pat) & pmask;
    for (u64 base = from; base <= last; base += 8 * TG) {        // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        u32 off = 8;                                             // byte of the own word where pat starts: 8 = nowhere
        if (p64 <= last) {
            const u32 p = (u32)p64;
            const u64 w = load_text8(ch.text + p), nxt = load_text8(ch.text + p + 8);
            u64 cand = zero_bytes(w ^ first);
            const u32 nv = last - p + 1;                         // start positions of this word inside the range
            if (nv < 8) cand &= (1ull << (8 * nv)) - 1ull;
            while (cand && off == 8) {
                const u32 k = (u32)(__builtin_ctzll(cand) >> 3);
                cand &= cand - 1;
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
                if ((x & pmask) == pk && (plen <= 8 || cmp_suffix(ch.text, ch.n, p + k, pat, plen) == 0)) off = k;
            }
        }
        // The ballots run while the groups of a wavefront are on different paths (other candidates, other segments, other
        // trip counts); a ballot counts the active lanes only, and only the group's own TG bits are read.  INVARIANT, as
        // in entry_holds: the TG lanes of a group reach every ballot together -- every branch between the kernel's loop
        // entry and a ballot depends on group-wide values only (t, len[t], ok, the anchors, plen, from, lim, base, and
        // `who` below, itself a ballot read through the group's bits), and the per-lane `p64 <= last` branch closes above.
        // The winning lane's byte offset reaches the group the same way: three more ballots over the bits of `off`, read at
        // the winner's bit.  (No shuffle: nothing here has to argue that a source lane is active.)
        const u32 who = (u32)(__ballot(off < 8) >> gbase) & ((1u << TG) - 1u);
        if (who) {
            const u32 wl = (u32)__builtin_ctz(who);              // the lowest lane that found one
            const u32 b0 = (u32)(__ballot((off & 1u) != 0) >> (gbase + wl)) & 1u;
            const u32 b1 = (u32)(__ballot((off & 2u) != 0) >> (gbase + wl)) & 1u;
            const u32 b2 = (u32)(__ballot((off & 4u) != 0) >> (gbase + wl)) & 1u;
            return (u32)base + 8 * wl + (b0 | (b1 << 1) | (b2 << 2));
        }
    }
    return kNone;
}

// TG lanes per hit the dedupe kept (one per candidate entry): the group's segments inside the entry [start, true end),
// in order.  The true end is the closing newline or n -- not start + len, which is short by one for an unterminated last
// entry.  An END anchor pins the last segment to the entry's end and a START anchor the first to its start; what is left
// is walked left to right, each segment at its LEFTMOST occurrence behind the one before it.  Leftmost-greedy is complete
// for patterns whose only wildcard is `*`: if any placement p_0 < p_1 < .. exists, moving p_0 to the leftmost occurrence
// of s_0 keeps every later constraint (p_1 >= p_0 + |s_0| only gets looser), and so on by induction -- no backtracking.
// The same shape as terms_verify_kernel, for the same reasons: TG = 8 lanes per candidate (64 bytes of entry per step),
// 32 candidates per 256-thread workgroup, grid-stride.
__global__ __launch_bounds__(256) void seq_verify_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                           const u64 *goff, const u8 *anchors, u64 ngq, const u64 *hit_off, u64 H,
                                                           const u32 *start, u32 *len)
{
    const u32 lane = lane_id(), gl = lane & (TG - 1), gbase = lane & ~(TG - 1);
    const u64 step = (u64)gridDim.x * blockDim.x / TG;
    for (u64 t = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / TG; t < H; t += step) {
        const u32 l = len[t];
        if (l == kSkip) continue;
        u64 a = 0, b = ngq;
        while (b - a > 1) {
            const u64 mid = a + (b - a) / 2;
            if (hit_off[mid] <= t) a = mid; else b = mid;
        }
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
            ok = pl == end - s && entry_find(ch, s, end, qbytes + qoff[j0], pl, gl, gbase) != kNone;
            j0 = j1;
        }
        if (ok && (anch & 2u) && j0 < j1) {                      // END: the last segment sits at the entry's end
            --j1;
            const u32 pl = (u32)(qoff[j1 + 1] - qoff[j1]);
            ok = pl <= end - s && entry_find(ch, end - pl, end, qbytes + qoff[j1], pl, gl, gbase) != kNone;
            if (ok) lim = end - pl;
        }
        if (ok && (anch & 1u) && j0 < j1) {                      // START: the first segment sits at the entry's start
            const u32 pl = (u32)(qoff[j0 + 1] - qoff[j0]);
            ok = pl <= lim - s && entry_find(ch, s, s + pl, qbytes + qoff[j0], pl, gl, gbase) != kNone;     // (lim >= s)
            from = s + pl;                                       // (ok: from <= lim, the two anchored segments do not overlap)
            ++j0;
        }
        for (u32 j = j0; j < j1 && ok; ++j) {
            const u32 pl = (u32)(qoff[j + 1] - qoff[j]);
            const u32 p = entry_find(ch, from, lim, qbytes + qoff[j], pl, gl, gbase);
            ok = p != kNone;
            from = p + pl;
        }
        if (!ok && gl == 0) len[t] = kSkip;
    }
}
