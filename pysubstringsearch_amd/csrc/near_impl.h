// near_impl.h -- entries that hold a pattern within k substituted bytes (Hamming distance; include/pss.h,
// pss_reader_search_near_batch).
// Part of search.hip: included there behind seed_impl.h, whose seeded verify path it gives the compare within a budget,
// and behind entry_scan_impl.h (TG, the group geometry); not a header for anybody else.
//
// The host cuts pattern p (L bytes, budget k < L) into k + 1 non-empty pieces, piece j = p[j L / (k + 1), (j + 1) L / (k + 1))
// (near_pieces below: what pss_near_pieces shows).  k mismatches cannot touch all k + 1 pieces, so every window within
// budget holds at least one piece exactly, at its offset.  The pieces are the seed queries of the pattern, its one term
// (seed_impl.h).  Pieces differ in length and may repeat (`abab`, k = 1) or nest (`aab` + `aa`): unlike spellings their
// intervals are neither disjoint nor ascending, so a (pattern, chunk) pair's hits are the plain sum of its pieces' counts,
// up to (k + 1) n -- why seed_union_kernel adds in 64 bits and a near batch passes it the overflow flag.  NearMatch::at
// lets a piece hit stand only as its alignment's FIRST EXACT PIECE, inside the hit's entry; NearMatch::before finds the
// entry's LEFTMOST window within budget.  Together: one hit per matching entry, the first exact piece of its leftmost near
// match.
// Bytes are exact (no fold) in the <false> forms below.  The <true> forms compare under ASCII case folding:
// the pattern is folded to lower case already, the text is folded on load (fold8 on 8-byte words), and a query is a
// spelling of the seed of a piece, not a piece -- see NearMatch<true>.
//
// Bounds: seed_impl.h states them for both kinds.  Near's own: near_count reads pat[from, to) and text[s + from, s + to)
// of a window the caller knows to end at or before n, 8 bytes a step with the tail masked, and near_scan's prefix compare
// reads its word and the one behind it -- both inside the 23 / 15 / 10 bytes stated there.

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

// Offset of piece j (0 .. np, np = k + 1 pieces) inside a pattern of plen bytes: near_pieces' j plen / np, computed where
// no query states it (under fold a query is a spelling of a piece's seed).  np is 1 .. 4; the product needs 34 bits.
__device__ __forceinline__ u32 piece_off(u32 j, u32 plen, u32 np)
{
    const u64 x = (u64)j * plen;
    return (u32)(np == 3 ? x / 3 : x >> (np >> 1));
}

// The piece that holds position sp of the pattern: the j with piece_off(j) <= sp < piece_off(j + 1).
__device__ __forceinline__ u32 piece_of(u32 sp, u32 plen, u32 np)
{
    u32 j = 0;
    for (u32 i = 1; i < np; ++i) j += piece_off(i, plen, np) <= sp ? 1u : 0u;      // (at most 3 trips)
    return j;
}

// Mismatches of pat[from, to) against text[s + from, s + to), added to `have`; gives up -- with a value above `budget` --
// as soon as the budget is exceeded.  8 bytes a step, the tail masked as in fold_equal.  The caller knows s + to <= n.
// kFold: the text word is folded before the xor (pat is folded already).
template <bool kFold>
__device__ __forceinline__ u32 near_count(const u8 *text, u32 s, const u8 *pat, u32 from, u32 to, u32 have, u32 budget)
{
    for (u32 i = from; i < to && have <= budget; i += 8) {
        const u64 tw = load_text8(text + s + i);
        u64 x = (kFold ? fold8(tw) : tw) ^ load_u64_unaligned(pat + i);
        const u32 rem = to - i;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        have += nonzero_bytes(x);
    }
    return have;
}

// Does a window within `budget` mismatches of pat (plen bytes) START in text[from, last] (from <= last, both inclusive)?
// The scan beside entry_scan, for the TG lanes of one group together: entry_scan's candidate filter -- the bytes equal to
// the pattern's first byte -- is wrong under a mismatch budget, where the first byte may be the one that differs.  Per
// 64-byte step lane gl takes the 8 start positions of its own 8-byte word; for each it counts the mismatches of the
// pattern's first min(8, plen) bytes in registers -- its word and the one behind it, shifted, as entry_scan forms x -- and
// goes back to memory for the rest (near_count) only when that prefix is within budget.  No position is read out:
// "whether" is all the dedupe asks, so the group agrees by ONE ballot read through its own TG bits.
// The TG lanes of a group reach the ballot together (the invariant of seed_dedupe_kernel): from, last, plen, budget and
// base are group-wide, and the per-lane `p64 <= last` branch, with the per-lane loop over the word's start positions
// inside it, closes before it.
// The caller knows that a window at `last` ends inside the chunk.  Loads reach at most 23 bytes past a start position and
// 15 past a compared range.  The loop is bounded by last - from, the inner ones by 8 and by plen: nothing spins.
// kFold: both text words are folded before the shifted xor; nothing else differs, the invariant and the bounds are the same.
template <bool kFold>
__device__ __forceinline__ bool near_scan(const ChunkDesc &ch, u32 from, u32 last, const u8 *pat, u32 plen, u32 budget, u32 gl, u32 gbase)
{
    const u64 pmask = plen >= 8 ? ~0ull : (1ull << (8 * plen)) - 1ull;
    const u64 pk = load_u64_unaligned(pat) & pmask;
    for (u64 base = from; base <= last; base += 8 * TG) {        // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        bool found = false;
        if (p64 <= last) {
            const u32 p = (u32)p64;
            const u64 w0 = load_text8(ch.text + p), nxt0 = load_text8(ch.text + p + 8);
            const u64 w = kFold ? fold8(w0) : w0, nxt = kFold ? fold8(nxt0) : nxt0;
            const u32 left = last - p + 1, nv = left < 8 ? left : 8u;        // start positions of this word inside the range
            for (u32 k = 0; k < nv && !found; ++k) {
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
                const u32 miss = nonzero_bytes((x ^ pk) & pmask);
                if (miss <= budget) found = plen <= 8 || near_count<kFold>(ch.text, p + k, pat, 8, plen, miss, budget) <= budget;
            }
        }
        if ((u32)(__ballot(found) >> gbase) & ((1u << TG) - 1u)) return true;
    }
    return false;
}

// The compare of the seeded path (seed_impl.h) within a budget.  The queries v0 .. v1 are the pattern's at most 4 pieces,
// piece w at T.pos[w] inside it; the hit came from piece v.  (The exact-byte form; NearMatch<true> is stated below.)
template <bool kFold>
struct NearMatch {
    static constexpr bool kFixedWindow = true;      // a mismatch moves nothing: the window is [di - pos, di - pos + L), as under fold
    // After the frame's reject (1. di >= pos and m + L <= n: the whole window is readable) the hit stands iff:
    //   2. the entry around di (a piece holds no newline, so it lies inside one entry) -- its TRUE end is the closing newline
    //      or n, not start + len, which is short by one for an unterminated last entry -- ...
    //   3. ... holds the window: m >= start and m + L <= end.  A window that leaves the entry is rejected even when the newline
    //      would be one of its at most k differing bytes (the step the case-insensitive search does not need: there a match
    //      holds no newline);
    //   4. text[m, m + L) differs from the pattern in at most k bytes, counted piece by piece (piece v itself is exact and is
    //      not read again);
    //   5. every piece before v holds a mismatch: else that piece is exact too, and the alignment's hit is ITS hit, not this
    //      one.  Without this an alignment that holds two pieces exactly would leave two hits and the dedupe would keep both.
    // 4 and 5 are EVALUATED before 2 and 3: a count is one or two loads where the entry's bounds are two 64-byte loads and a
    // scan, and of the k + 1 candidates an exact occurrence leaves, k fall to 5.
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 v0, u32 v1, u32 v, u32 di, u32 &m, u32 plen,
                                              u32 &ls, u32 &ll)
    {
        const u32 budget = T.budget[g];
        const u8 *pat = T.bytes + T.off[g];
        u32 miss = 0;
        bool first = true;
        for (u32 w = v0; w < v1 && first && miss <= budget; ++w) {              // (at most 4 pieces)
            if (w == v) continue;
            const u32 before = miss;
            miss = near_count<false>(ch.text, m, pat, T.pos[w], w + 1 < v1 ? T.pos[w + 1] : plen, miss, budget);
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
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32 plen, u32 gl,
                                                  u32 gbase, u32)
    {
        return near_scan<false>(ch, from, last, T.bytes + T.off[g], plen, T.budget[g], gl, gbase);
    }
};

// The same compare under ASCII case folding.  The pattern is folded to lower case; its queries v0 .. v1
// are, piece by piece, the spellings of the piece's SEED (at most 64 in all), so T.pos[v] is the seed's position inside the
// pattern and states no piece bounds: they are computed (piece_off), and the hit's piece j is the one that holds T.pos[v].
// After the frame's reject (di >= pos and m + L <= n with m = di - pos: the whole window is readable), in this order:
//   1. piece j is fold-equal over its WHOLE length -- the seed guarantees only its own bytes;
//   2. every piece before j holds a folded mismatch (else the alignment's hit is that piece's: its seed stands there in
//      exactly one spelling, which is a query too);
//   3. the folded mismatches of the whole window are within the budget;
//   4. the entry around di holds the window (a seed holds no newline; the entry's true end as in the exact form).
// Together with near_scan<true> in front of m: one hit per matching entry, in one spelling of the seed of the first
// fold-exact piece of its leftmost window within budget.  Bounds and the group-wide-ballot invariant are the exact form's
// (seed_impl.h): every read lies in the window [m, m + L) inside [0, n), every tail is masked, the loops are bounded by the
// 4 pieces and by L; before() passes group-wide arguments only.  No LDS, no scratch.
template <>
struct NearMatch<true> {
    static constexpr bool kFixedWindow = true;
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32, u32, u32 v, u32 di, u32 &m, u32 plen,
                                              u32 &ls, u32 &ll)
    {
        const u32 budget = T.budget[g], np = budget + 1;
        const u8 *pat = T.bytes + T.off[g];
        const u32 j = piece_of(T.pos[v], plen, np);
        if (near_count<true>(ch.text, m, pat, piece_off(j, plen, np), piece_off(j + 1, plen, np), 0, 0)) return;
        u32 miss = 0;
        bool first = true;
        for (u32 w = 0; w < np && first && miss <= budget; ++w) {               // (at most 4 pieces)
            if (w == j) continue;
            const u32 before = miss;
            miss = near_count<true>(ch.text, m, pat, piece_off(w, plen, np), piece_off(w + 1, plen, np), miss, budget);
            first = w > j || miss != before;
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
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32 plen, u32 gl,
                                                  u32 gbase, u32)
    {
        return near_scan<true>(ch, from, last, T.bytes + T.off[g], plen, T.budget[g], gl, gbase);
    }
};
