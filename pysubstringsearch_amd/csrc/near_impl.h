// near_impl.h -- entries that hold a pattern within k substituted bytes (Hamming distance; include/pss.h,
// pss_reader_search_near_batch).
// Part of search.hip: included there behind fold_impl.h, whose three-level pipeline it reruns with other words --
// group -> term -> spellings of a seed becomes pattern -> pattern -> its k + 1 PIECES -- and behind entry_scan_impl.h
// (TG, the group geometry); not a header for anybody else.
//
// The host cuts pattern p (L bytes, budget k < L) into k + 1 non-empty pieces, piece j = p[j L / (k + 1), (j + 1) L / (k + 1))
// (near_pieces below: what pss_near_pieces shows).  k mismatches cannot touch all k + 1 pieces, so every window within
// budget holds at least one piece exactly, at its offset.  The pieces are the queries of the staged request: the interval
// kernels answer every (piece, chunk) pair unchanged.  Pieces differ in length and may repeat (`abab`, k = 1) or nest
// (`aab` + `aa`): unlike spellings their intervals are neither disjoint nor ascending, so a (pattern, chunk) pair's hits
// are the plain sum of its pieces' counts, up to (k + 1) n -- near_union_kernel adds in 64 bits and flags a pair past
// 2^32 - 1 instead of wrapping.  terms_driver_kernel<false> picks every pair's one term.  near_hits_kernel verifies the
// whole pattern around each piece hit inside the hit's entry and lets the hit stand only as its alignment's FIRST EXACT
// PIECE; near_dedupe_kernel keeps the hit of the entry's LEFTMOST window within budget.  Together: one hit per matching
// entry, the first exact piece of its leftmost near match.  The kept-hit scan, the counts and the two emit kernels run as
// always.
// Bytes are exact (no fold); a pattern that holds a 0x0A occurs in no entry and is flagged void: its pairs count no hit.
//
// Bounds, for both kernels.  A window that is read lies in [0, n): near_hits_kernel rejects di < off and m + L > n before
// it reads, and every window the dedupe looks at starts before m and so ends before m + L <= n.  Text loads are
// load_text8 at a byte of such a window or 8 past a start position: at most 23 bytes past a start position and 15 past a
// compared range (the text is readable 128 bytes past n).  A pattern is read by load_u64_unaligned at one of its bytes: at
// most 10 bytes past its end (32 zero bytes follow the patterns on the device).  The tail of every compare is masked, so
// a 0x00 at a pattern's end is never taken as equal to that padding, nor a text byte behind the window as part of it.
// The two kernels write start[t], len[t], m[t] of their own hit t and nothing else.  No LDS, no scratch.

// The k + 1 pieces of a pattern of len > k bytes: piece j is [off[j], off[j + 1]), off[k + 1] = len.  (Host code, declared
// in search.h: the C ABI expands the patterns before it states the request.)
void near_pieces(u64 len, u32 k, u64 *off)
{
    for (u32 j = 0; j <= k + 1; ++j) off[j] = (u64)j * len / (k + 1);
}

// High bit of every byte of x that is NOT zero (exact, no cross-byte carries): the popcount is the Hamming distance of the
// two 8-byte words x is the xor of.
__device__ __forceinline__ u32 nonzero_bytes(u64 x)
{
    const u64 m = 0x7f7f7f7f7f7f7f7full;
    return (u32)__popcll((((x & m) + m) | x) & ~m);
}

// Mismatches of pat[from, to) against text[s + from, s + to), added to `have`; gives up -- with a value above `budget` --
// as soon as the budget is exceeded.  8 bytes a step, the tail masked as in fold_equal.  The caller knows s + to <= n.
__device__ __forceinline__ u32 near_count(const u8 *text, u32 s, const u8 *pat, u32 from, u32 to, u32 have, u32 budget)
{
    for (u32 i = from; i < to && have <= budget; i += 8) {
        u64 x = load_text8(text + s + i) ^ load_u64_unaligned(pat + i);
        const u32 rem = to - i;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        have += nonzero_bytes(x);
    }
    return have;
}

// One lane per (pattern, chunk) pair: the hits of the pair are the hits of its pieces, one interval behind the other.
// The intervals may overlap or repeat, so the sum can reach (k + 1) n: it is taken in 64 bits, and THIS is where a pair of
// more than 2^32 - 1 hits is caught -- the pair counts 0 and raises *over, which fails the batch on the host before any
// hit buffer is reserved (Batch::run_general).
__global__ __launch_bounds__(256) void near_union_kernel(u32 nc, const u64 *soff, const u8 *fvoid, const u32 *cnt, u64 ngq, u32 *p_cnt,
                                                           u64 *over)
{
    const u64 gq = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gq >= ngq) return;
    const u32 g = (u32)(gq / nc), c = (u32)(gq % nc);
    u64 sum = 0;
    if (!fvoid[g])
        for (u32 v = (u32)soff[g], v1 = (u32)soff[g + 1]; v < v1; ++v) sum += cnt[(u64)v * nc + c];
    if (sum > 0xffffffffull) {
        *over = 1;
        sum = 0;
    }
    p_cnt[gq] = (u32)sum;
}

// One lane per hit; the shape of fold_hits_kernel.  The pairs are (pattern, chunk) pairs and the pattern of pair a is its
// one term g_drv[a]; soff (the piece offsets into the queries), foff, nk are indexed by pattern, poff by piece.  Hit k' of
// a pair is suffix sa[lo[v, c] + k''] of the piece v = soff[g] + j its walk over the pattern's at most 4 counts ends in.
// With di that text offset the window would start at m = di - off_j.  The hit stands iff all of these hold:
//   1. di >= off_j and m + L <= n: else it is rejected before anything is read;
//   2. the entry around di (a piece holds no newline, so it lies inside one entry) -- its TRUE end is the closing newline
//      or n, not start + len, which is short by one for an unterminated last entry -- ...
//   3. ... holds the window: m >= start and m + L <= end.  A window that leaves the entry is rejected even when the newline
//      would be one of its at most k differing bytes (the step the case-insensitive search does not need: there a match
//      holds no newline);
//   4. text[m, m + L) differs from the pattern in at most k bytes, counted piece by piece (piece j itself is exact and is
//      not read again);
//   5. every piece j' < j holds a mismatch: else that piece is exact too, and the alignment's hit is ITS hit, not this
//      one.  Without this an alignment that holds two pieces exactly would leave two hits and the dedupe would keep both.
// 4 and 5 are EVALUATED before 2 and 3: after 1 the whole window is readable, a count is one or two loads where the
// entry's bounds are two 64-byte loads and a scan, and of the k + 1 candidates an exact occurrence leaves, k fall to 5.
// A surviving hit leaves start, len and m.
__global__ __launch_bounds__(256) void near_hits_kernel(const ChunkDesc *chunks, u32 nc, const u8 *fbytes, const u64 *foff, const u8 *nk,
                                                          const u32 *poff, const u64 *soff, const u32 *lo, const u32 *cnt, u64 ngq,
                                                          const u64 *hit_off, u64 H, u32 *start_out, u32 *len_out, u32 *m_out, const u32 *g_drv)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a], c = (u32)(a % nc);
        const ChunkDesc ch = chunks[c];
        u32 k = (u32)(t - hit_off[a]);
        const u32 v0 = (u32)soff[g], v1 = (u32)soff[g + 1];
        u32 v = v0;
        for (; v + 1 < v1; ++v) {                                // (k < the pair's sum: the walk ends inside [v0, v1))
            const u32 n_v = cnt[(u64)v * nc + c];
            if (k < n_v) break;
            k -= n_v;
        }
        const u32 di = ch.sa[lo[(u64)v * nc + c] + k];
        const u32 off = poff[v], plen = (u32)(foff[g + 1] - foff[g]), budget = nk[g];
        const u8 *pat = fbytes + foff[g];
        u32 ls = 0, ll = kSkip, m = 0;
        if (di >= off && (u64)(di - off) + plen <= ch.n) {
            m = di - off;
            u32 miss = 0;
            bool first = true;
            for (u32 w = v0; w < v1 && first && miss <= budget; ++w) {              // (at most 4 pieces)
                if (w == v) continue;
                const u32 before = miss;
                miss = near_count(ch.text, m, pat, poff[w], w + 1 < v1 ? poff[w + 1] : plen, miss, budget);
                first = w > v || miss != before;
            }
            if (first && miss <= budget) {
                u32 es, el;
                entry_bounds(ch, di, es, el);
                const u32 end = ch.text[es + el] == '\n' ? es + el : ch.n;
                if (m >= es && m + plen <= end) {
                    ls = es;
                    ll = el;
                }
            }
        }
        start_out[t] = ls;
        len_out[t] = ll;
        m_out[t] = m;
    }
}

// Does a window within `budget` mismatches of pat (plen bytes) START in text[from, last] (from <= last, both inclusive)?
// The scan beside entry_scan, for the TG lanes of one group together: entry_scan's candidate filter -- the bytes equal to
// the pattern's first byte -- is wrong under a mismatch budget, where the first byte may be the one that differs.  Per
// 64-byte step lane gl takes the 8 start positions of its own 8-byte word; for each it counts the mismatches of the
// pattern's first min(8, plen) bytes in registers -- its word and the one behind it, shifted, as entry_scan forms x -- and
// goes back to memory for the rest (near_count) only when that prefix is within budget.  No position is read out:
// "whether" is all the dedupe asks, so the group agrees by ONE ballot read through its own TG bits.
// INVARIANT (entry_scan's, restated at this ballot): the TG lanes of a group reach the ballot together -- every branch
// between the calling kernel's loop entry and the ballot depends on group-wide values only (the hit t and what is read at
// t, the pair and its pattern, from, last, plen, budget, base), and the per-lane `p64 <= last` branch, with the per-lane
// loop over the word's start positions inside it, closes before it.
// The caller knows that a window at `last` ends inside the chunk.  Loads reach at most 23 bytes past a start position and
// 15 past a compared range.  The loop is bounded by last - from, the inner ones by 8 and by plen: nothing spins.
__device__ __forceinline__ bool near_scan(const ChunkDesc &ch, u32 from, u32 last, const u8 *pat, u32 plen, u32 budget, u32 gl, u32 gbase)
{
    const u64 pmask = plen >= 8 ? ~0ull : (1ull << (8 * plen)) - 1ull;
    const u64 pk = load_u64_unaligned(pat) & pmask;
    for (u64 base = from; base <= last; base += 8 * TG) {        // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        bool found = false;
        if (p64 <= last) {
            const u32 p = (u32)p64;
            const u64 w = load_text8(ch.text + p), nxt = load_text8(ch.text + p + 8);
            const u32 left = last - p + 1, nv = left < 8 ? left : 8u;        // start positions of this word inside the range
            for (u32 k = 0; k < nv && !found; ++k) {
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
                const u32 miss = nonzero_bytes((x ^ pk) & pmask);
                if (miss <= budget) found = plen <= 8 || near_count(ch.text, p + k, pat, 8, plen, miss, budget) <= budget;
            }
        }
        if ((u32)(__ballot(found) >> gbase) & ((1u << TG) - 1u)) return true;
    }
    return false;
}

// TG lanes per hit that near_hits_kernel left standing; the shape of fold_dedupe_kernel (64 bytes of entry per step, 32
// hits per 256-thread workgroup, grid-stride).  The hit is kept iff NO window within budget starts in [start, m).  Such a
// window may overlap m; it ends before m + L, hence inside the entry and the chunk.  Every loop is bounded by m - start,
// by L or by 8.  The pattern of pair a is its one term g_drv[a] -- one value per hit, so near_scan's invariant holds.
__global__ __launch_bounds__(256) void near_dedupe_kernel(const ChunkDesc *chunks, u32 nc, const u8 *fbytes, const u64 *foff, const u8 *nk,
                                                            u64 ngq, const u64 *hit_off, u64 H, const u32 *start, const u32 *mpos, u32 *len,
                                                            const u32 *g_drv)
{
    const u32 lane = lane_id(), gl = lane & (TG - 1), gbase = lane & ~(TG - 1);
    const u64 step = (u64)gridDim.x * blockDim.x / TG;
    for (u64 t = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / TG; t < H; t += step) {
        if (len[t] == kSkip) continue;
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a];
        const ChunkDesc ch = chunks[(u32)(a % nc)];
        const u32 s = start[t], m = mpos[t];
        const bool dup = m > s && near_scan(ch, s, m - 1, fbytes + foff[g], (u32)(foff[g + 1] - foff[g]), nk[g], gl, gbase);
        if (dup && gl == 0) len[t] = kSkip;
    }
}
