// all_terms_impl.h -- entries that contain ALL the include terms of a group and NONE of its exclude terms (include/pss.h,
// pss_reader_search_terms_batch).
// Part of search.hip: included there behind the entry helpers (cmp_suffix, load_text8, hit_entry) and the workspace slots;
// not a header for anybody else.
//
// A batch of ng groups over nterms terms has TWO pair spaces:
//   term pairs   (term, chunk), nterms x nc: what the interval kernels of search.hip answer, unchanged -- lo and count of
//                every term in every chunk before a single hit is touched;
//   group pairs  (group, chunk), ng x nc: what everything from the first scan on runs over.
// terms_driver_kernel joins them: per group pair it picks the include term with the fewest hits in that chunk (the
// lowest index on a tie) and hands its interval on as the pair's.  A chunk where an include term is absent counts zero
// hits for the pair.  terms_hits_kernel is hit_lines_kernel with the driver's pattern: leftmost-match dedupe and entry
// bounds, one candidate per entry that holds the driver.  terms_verify_kernel then scans each candidate entry once for
// the group's other terms and marks it kSkip when an include term is missing or an exclude term is there; the kept-hit
// scan, the counts and the two emit kernels of the general pipeline run as always.
// A term that holds a 0x0A occurs in no entry, but its interval need not be empty (it may match across entries): such a
// term is flagged on the host.  As an include term it voids its group, as an exclude term it is ignored.

constexpr u8 kTermExclude = 1;
constexpr u8 kTermVoid = 0x80;                   // the term holds a newline: it occurs in no entry
constexpr u32 TG = 8;                            // lanes per candidate entry in terms_verify_kernel: 64 bytes per step

// Per-term flags of a batch (nterms values).
static void terms_flags(const u8 *qbytes, const u64 *qoff, u32 nterms, const u8 *exclude, u8 *flags)
{
    for (u32 t = 0; t < nterms; ++t) {
        const u64 m = qoff[t + 1] - qoff[t];
        flags[t] = (u8)((exclude[t] ? kTermExclude : 0) | ((m && memchr(qbytes + qoff[t], '\n', m)) ? kTermVoid : 0));
    }
}

// One lane per (group, chunk) pair: the driver term of the pair, its interval and its hit count.
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
    g_lo[gq] = have ? lo[(u64)bt * nc + c] : 0u;
    g_cnt[gq] = (have && !dead) ? best : 0u;
}

// hit_lines_kernel over the group pairs: hit k of a pair is suffix sa[lo + k] of its driver's interval, and the driver's
// pattern decides which hit of an entry is the leftmost.
__global__ __launch_bounds__(256) void terms_hits_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                           const u32 *g_drv, u64 ngq, const u32 *g_lo, const u64 *hit_off, u64 H,
                                                           u32 *start_out, u32 *len_out)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        u64 a = 0, b = ngq;
        while (b - a > 1) {
            const u64 mid = a + (b - a) / 2;
            if (hit_off[mid] <= t) a = mid; else b = mid;
        }
        const ChunkDesc ch = chunks[(u32)(a % nc)];
        const u32 q = g_drv[a];
        const u8 *pat = qbytes + qoff[q];
        const u32 plen = (u32)(qoff[q + 1] - qoff[q]);
        const u32 di = ch.sa[g_lo[a] + (u32)(t - hit_off[a])];
        u32 ls = 0, ll = 0;
        if (hit_entry(ch, pat, plen, di, ls, ll)) {
            start_out[t] = ls;
            len_out[t] = ll;
        } else {
            start_out[t] = 0;
            len_out[t] = kSkip;
        }
    }
}

// Does text[s, end) hold pat?  Called by the TG lanes of one group together (gl = lane inside the group, gbase = the
// group's first lane); every lane returns the group's answer.  A match starts at s .. end - plen and nowhere else, so it
// never reaches the newline at `end`, the next entry or the zero padding behind the chunk.  Per step the group covers
// 8 * TG start positions: lane gl takes the 8 that begin at its own 8-byte word, finds the bytes equal to the term's
// first byte (zero_bytes) and checks those against the term's first min(8, plen) bytes in registers; only a term longer
// than 8 bytes whose first 8 match goes back to memory.  Loads reach at most 23 bytes past a start position (the text is
// readable 128 bytes past n, a term 16 past its end).
__device__ __forceinline__ bool entry_holds(const ChunkDesc &ch, u32 s, u32 end, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    if (plen > end - s) return false;
    const u32 last = end - plen;                                 // the last start position
    const u64 first = 0x0101010101010101ull * pat[0];
    const u64 pmask = plen >= 8 ? ~0ull : (1ull << (8 * plen)) - 1ull;
    const u64 pk = load_u64_unaligned(pat) & pmask;
    for (u64 base = s; base <= last; base += 8 * TG) {           // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        bool found = false;
        if (p64 <= last) {
            const u32 p = (u32)p64;
            const u64 w = load_text8(ch.text + p), nxt = load_text8(ch.text + p + 8);
            u64 cand = zero_bytes(w ^ first);
            const u32 nv = last - p + 1;                         // start positions of this word inside the entry
            if (nv < 8) cand &= (1ull << (8 * nv)) - 1ull;
            while (cand && !found) {
                const u32 k = (u32)(__builtin_ctzll(cand) >> 3);
                cand &= cand - 1;
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
                if ((x & pmask) == pk) found = plen <= 8 || cmp_suffix(ch.text, ch.n, p + k, pat, plen) == 0;
            }
        }
        // The ballot runs while the groups of a wavefront are on different paths (other candidates, other terms, other
        // trip counts); it counts the active lanes only, and only the group's own TG bits are read.  INVARIANT: the TG
        // lanes of a group reach every ballot together -- every branch between the kernel's loop entry and this line
        // depends on group-wide values only (t, len[t], ok, plen, s, end, base), and the per-lane `p64 <= last` branch
        // closes above.  A lane that took a path of its own would split the group's ballot, and the lanes would disagree.
        if ((u32)(__ballot(found) >> gbase) & ((1u << TG) - 1u)) return true;
    }
    return false;
}

// TG lanes per hit the dedupe kept (one per candidate entry): the group's other terms inside the entry [start, true
// end).  The true end is the closing newline or n -- not start + len, which is short by one for an unterminated last
// entry.  An exclude term without a hit in the chunk cannot be in the entry and is not looked for.
__global__ __launch_bounds__(256) void terms_verify_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                             const u64 *goff, const u8 *flags, const u32 *cnt, const u32 *g_drv,
                                                             u64 ngq, const u64 *hit_off, u64 H, const u32 *start, u32 *len)
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
        const u32 drv = g_drv[a], t1 = (u32)goff[g + 1];
        bool ok = true;
        for (u32 j = (u32)goff[g]; j < t1 && ok; ++j) {
            const u8 f = flags[j];
            const bool excl = (f & kTermExclude) != 0;
            if (j == drv || (f & kTermVoid)) continue;           // (a void include term left the pair without hits)
            if (excl && cnt[(u64)j * nc + c] == 0) continue;
            const bool found = entry_holds(ch, s, end, qbytes + qoff[j], (u32)(qoff[j + 1] - qoff[j]), gl, gbase);
            ok = found != excl;
        }
        if (!ok && gl == 0) len[t] = kSkip;
    }
}
