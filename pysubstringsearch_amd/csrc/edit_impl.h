// edit_impl.h -- entries that hold a pattern within k edited bytes (Levenshtein distance: insertions, deletions and
// substitutions of single bytes; include/pss.h, pss_reader_search_edit_batch).
// Part of search.hip: included there behind near_impl.h, whose pieces, seed queries and budgets it shares, and behind
// seed_impl.h, whose seeded verify path it gives the third compare; not a header for anybody else.
//
// The pieces are near's (near_pieces): k edits cannot touch all k + 1 of them, so every substring w of an entry with
// lev(w, p) <= k holds some piece j exactly.  Unlike a mismatch an edit shifts what stands behind it, so the piece need
// not stand at its offset inside w and a hit names no window.  A CANDIDATE is (piece j, exact occurrence at text offset d);
// with off / len the piece's offset and length inside p it STANDS iff lc + rc <= k, where
//   lc = the least lev(text[a, d), p[0, off)) over a in [entry start, d] and
//   rc = the least lev(text[d + len, b), p[off + len, L)) over b in [d + len, entry end].
// The two sides are independent: the left is computed within k, the right within k - lc (edit_side).  An entry matches iff
// one of its candidates stands, and the ONE hit kept for it is the standing candidate with the smallest d and, among
// equal d (one piece a prefix of the other, `aab` + `aa`), the smallest j: EditMatch::at lets a hit stand only when no
// earlier piece stands at the same d, EditMatch::before asks for a standing candidate in front of d.
// Bytes are exact (no fold) in the <false> forms below.  The <true> forms compare under ASCII case folding:
// the pattern is folded to lower case already and the text is folded on load -- fold8 on 8-byte words, one byte in
// edit_side's fetch --, and a query is a spelling of the seed of a piece, not a piece: see EditMatch<true>.
//
// Bounds.  edit_side reads the text one byte at a time, at an index it has checked to lie in [0, n), and stops at the
// first index that does not or that holds a 0x0A (a WALL): it needs no entry bounds, never reads below 0 and never takes a
// byte of the padding behind n for text.  It reads the pattern one byte at a time inside [0, L).  piece_at compares a piece
// it has checked to end at or before n, 8 bytes a step with the tail masked (load_text8: at most 15 bytes past the
// compared range; load_u64_unaligned: at most 7 past the piece, 32 zero bytes follow the terms).  edit_scan's prefix
// compare reads its word and the one behind it as near_scan does: at most 23 bytes past a start position below n.
// No LDS, no scratch: the band of the DP and its text window are named registers.

constexpr u32 kEditInf = 64;                // above every budget and every cell that counts
constexpr u32 kEditWall = 0x100;            // (no byte: the entry ends here)
constexpr u32 kEditNone = 0x200;            // (no byte: in front of the side's first one)

// One cell of the band: D[i][t] from its three neighbours.  w is the text byte of column t (T[t - 1]), pc the pattern
// byte of row i.  A column at or behind a wall does not exist; a value above the budget can only grow and is dropped,
// which is also what keeps the cells outside |i - t| <= budget out of the band.
__device__ __forceinline__ u32 edit_cell(u32 left, u32 diag, u32 up, u32 w, u32 pc, u32 budget)
{
    u32 v = diag + (w != pc ? 1u : 0u);
    v = min(v, min(up, left) + 1u);
    return (w == kEditWall || v > budget) ? kEditInf : v;
}

// One side of a candidate: the least lev(T[0, t), P) over t, where P is the side's m pattern bytes and T the text walked
// away from the piece until a wall -- kBack: T[t] = text[at - 1 - t] and P[i] = pat[m - 1 - i] (the left side, read
// right to left), else T[t] = text[at + t] and P[i] = pat[i] (the right side).  A value above `budget` (<= 3) comes back
// as kEditInf.  Row i of the DP (i pattern bytes taken) lives in r0 .. r6, columns t = i - 3 .. i + 3, and w0 .. w6 are
// the text bytes of those columns; a row shifts the window by one byte.  The loop ends at m or as soon as a whole row
// is above the budget: at most L trips of 7 cells.
// kFold: the text byte is folded to lower case as it is fetched (a newline is none of A-Z: the walls are unchanged).
template <bool kBack, bool kFold>
__device__ __forceinline__ u32 edit_side(const u8 *text, u32 n, u32 at, const u8 *pat, u32 m, u32 budget)
{
    if (m == 0) return 0;
    u32 taken = 0;
    bool wall = false;
    // The next byte of the side, or a wall; a wall stays a wall.  No branch (each would cost the divergent callers a lane
    // mask): the index is judged first, and a lane whose index is no text, or that stands at a wall already, loads byte 0
    // of the chunk instead (n > 0: the chunk holds a hit) and drops what it loaded.
    auto next = [&]() -> u32 {
        const bool in = !wall && (kBack ? taken < at : (u64)at + taken < n);
        const u32 idx = in ? (kBack ? at - 1 - taken : at + taken) : 0u;
        const u32 b0 = text[idx];
        const u32 b = kFold && b0 - 'A' < 26u ? b0 | 0x20u : b0;
        wall = !in || b == '\n';
        taken += wall ? 0u : 1u;
        return wall ? kEditWall : b;
    };
    u32 w0 = kEditNone, w1 = kEditNone, w2 = kEditNone, w3 = next(), w4 = next(), w5 = next(), w6 = next();
    // row 0: D[0][t] = t where the text has t bytes
    u32 r0 = kEditInf, r1 = kEditInf, r2 = kEditInf, r3 = 0;
    u32 r4 = (w3 != kEditWall && budget >= 1) ? 1u : kEditInf;
    u32 r5 = (w4 != kEditWall && budget >= 2) ? 2u : kEditInf;
    u32 r6 = (w5 != kEditWall && budget >= 3) ? 3u : kEditInf;
    for (u32 i = 1; i <= m; ++i) {
        if (i > 1) {
            w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6;
            w6 = next();
        }
        const u32 pc = pat[kBack ? m - i : i - 1];
        const u32 c0 = edit_cell(kEditInf, r0, r1, w0, pc, budget);
        const u32 c1 = edit_cell(c0, r1, r2, w1, pc, budget);
        const u32 c2 = edit_cell(c1, r2, r3, w2, pc, budget);
        const u32 c3 = edit_cell(c2, r3, r4, w3, pc, budget);
        const u32 c4 = edit_cell(c3, r4, r5, w4, pc, budget);
        const u32 c5 = edit_cell(c4, r5, r6, w5, pc, budget);
        const u32 c6 = edit_cell(c5, r6, kEditInf, w6, pc, budget);
        r0 = c0; r1 = c1; r2 = c2; r3 = c3; r4 = c4; r5 = c5; r6 = c6;
        if (min(min(min(r0, r1), min(r2, r3)), min(min(r4, r5), r6)) > budget) return kEditInf;
    }
    return min(min(min(r0, r1), min(r2, r3)), min(min(r4, r5), r6));
}

// Does the candidate (piece [off, off + len) of pat, exact at d) stand?
template <bool kFold>
__device__ __forceinline__ bool edit_stands(const ChunkDesc &ch, const u8 *pat, u32 plen, u32 off, u32 len, u32 d, u32 budget)
{
    const u32 lc = edit_side<true, kFold>(ch.text, ch.n, d, pat, off, budget);
    if (lc > budget) return false;
    return edit_side<false, kFold>(ch.text, ch.n, d + len, pat + off + len, plen - off - len, budget - lc) <= budget - lc;
}

// Is text[d + from, d + len) the piece's bytes [from, len)?  The piece must end inside the text: behind n stands zero
// padding, which a piece that ends in 0x00 bytes would else be found in.  kFold: the text word is folded before the xor.
template <bool kFold>
__device__ __forceinline__ bool piece_at(const ChunkDesc &ch, u32 d, const u8 *piece, u32 from, u32 len)
{
    if ((u64)d + len > ch.n) return false;
    for (u32 i = from; i < len; i += 8) {
        const u64 tw = load_text8(ch.text + d + i);
        u64 x = (kFold ? fold8(tw) : tw) ^ load_u64_unaligned(piece + i);
        const u32 rem = len - i;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        if (x) return false;
    }
    return true;
}

// Does a standing candidate of the pattern lie at some d' in text[from, last] (from <= last, both inclusive, inside one
// entry and below n)?  The shape of near_scan, for the TG lanes of one group together: per 64-byte step lane gl takes the
// 8 start positions of its own 8-byte word and compares, in registers, the first min(8, len) bytes of each of the at
// most 4 pieces with the text there -- its word and the one behind it, shifted.  Only a piece whose prefix is equal goes
// to memory for its rest (piece_at) and only an exact piece runs the two DPs (edit_stands): per lane and divergent, which
// is accepted because a piece occurs rarely inside one entry of real text (Limits).
// The TG lanes of a group reach the ballot together (the invariant of seed_dedupe_kernel): from, last, the pattern, its
// budget and base are group-wide, and everything that depends on gl -- the `p64 <= last` branch, the loop over the word's
// start positions, the loop over the pieces whose prefix is equal and the DPs inside it -- closes before the ballot.
// The loop is bounded by last - from, the inner ones by 8, by 4 and by the pattern's length: nothing spins.
// kFold: both text words are folded before the candidate mask is formed, and the pieces' offsets are computed (piece_off:
// `pos` is not read, under fold a query is no piece) -- arithmetic on group-wide values, so the invariant stands as it is.
template <bool kFold>
__device__ __forceinline__ bool edit_scan(const ChunkDesc &ch, u32 from, u32 last, const u8 *pat, u32 plen, const u32 *pos, u32 budget,
                                          u32 gl, u32 gbase)
{
    const u32 np = budget + 1;
    auto off_of = [&](u32 j) -> u32 { return kFold ? piece_off(j, plen, np) : pos[j]; };
    u64 pk[4], pm[4];
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {                                 // (constant indices: registers)
        pk[j] = 0;
        pm[j] = 0;
        if (j < np) {
            const u32 off = off_of(j), len = (j + 1 < np ? off_of(j + 1) : plen) - off;
            pm[j] = len >= 8 ? ~0ull : (1ull << (8 * len)) - 1ull;
            pk[j] = load_u64_unaligned(pat + off) & pm[j];
        }
    }
    for (u64 base = from; base <= last; base += 8 * TG) {        // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        bool found = false;
        if (p64 <= last) {
            const u32 p = (u32)p64;
            const u64 w0 = load_text8(ch.text + p), nxt0 = load_text8(ch.text + p + 8);
            const u64 w = kFold ? fold8(w0) : w0, nxt = kFold ? fold8(nxt0) : nxt0;
            const u32 left = last - p + 1, nv = left < 8 ? left : 8u;        // start positions of this word inside the range
            // bit 4 k + j: the first bytes of piece j stand at start position k of this word (straight-line code: one
            // loop less around the DPs, whose lane masks the scalar registers have to hold)
            u32 cand = 0;
#pragma unroll
            for (u32 k = 0; k < 8; ++k) {
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
#pragma unroll
                for (u32 j = 0; j < 4; ++j) cand |= (j < np && ((x ^ pk[j]) & pm[j]) == 0) ? 1u << (4 * k + j) : 0u;
            }
            if (nv < 8) cand &= (1u << (4 * nv)) - 1u;
            while (cand && !found) {                              // (rare: ascending positions, and pieces inside one)
                const u32 bit = (u32)__builtin_ctz(cand), k = bit >> 2, j = bit & 3;
                cand &= cand - 1;
                const u32 off = off_of(j), len = (j + 1 < np ? off_of(j + 1) : plen) - off;
                if (piece_at<kFold>(ch, p + k, pat + off, len < 8 ? len : 8u, len)) found = edit_stands<kFold>(ch, pat, plen, off, len, p + k, budget);
            }
        }
        if ((u32)(__ballot(found) >> gbase) & ((1u << TG) - 1u)) return true;
    }
    return false;
}

// The compare of the seeded path (seed_impl.h) within a budget of edits.  The queries v0 .. v1 are the pattern's at most 4
// pieces, piece w at T.pos[w] inside it; the hit came from piece v, which is exact at di by construction.  (The exact-byte
// form; EditMatch<true> is stated below.)
template <bool kFold>
struct EditMatch {
    // An edit moves what stands behind it: the match around a piece hit neither starts at di - pos nor ends at
    // di - pos + L, so the frame rejects nothing, passes di through as m, and m_out[t] is di -- the position the dedupe
    // looks before.
    static constexpr bool kFixedWindow = false;
    // The hit stands iff its candidate stands and no piece before v is exact at di and stands there too (the alignment's hit
    // is then THAT piece's).  The earlier pieces are judged first and through the same call as the hit's own: a piece in front
    // of v is exact at di only when it is a prefix of piece v or piece v of it, which one or two loads rule out.
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 v0, u32 v1, u32 v, u32 di, u32 &m, u32 plen,
                                              u32 &ls, u32 &ll)
    {
        const u32 budget = T.budget[g];
        const u8 *pat = T.bytes + T.off[g];
        bool ok = false;
        for (u32 w = v0; w <= v; ++w) {                           // (at most 4 pieces)
            const u32 off = T.pos[w], len = (w + 1 < v1 ? T.pos[w + 1] : plen) - off;
            if (w < v && !piece_at<false>(ch, di, pat + off, 0, len)) continue;
            const bool st = edit_stands<false>(ch, pat, plen, off, len, di, budget);
            if (w < v && st) break;
            ok = st;
        }
        if (ok) entry_bounds(ch, di, ls, ll);
    }
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32 plen, u32 gl,
                                                  u32 gbase, u32)
    {
        return edit_scan<false>(ch, from, last, T.bytes + T.off[g], plen, T.pos + (u32)T.soff[g], T.budget[g], gl, gbase);
    }
};

// The same compare under ASCII case folding.  The pattern is folded to lower case; its queries are, piece
// by piece, the spellings of the piece's SEED, so the hit at di says where the seed stands, not where its piece would: with
// j the piece that holds T.pos[v] (piece_of; the bounds are computed, piece_off) the CANDIDATE position is
// d = di - (T.pos[v] - off_j).  d < 0 or a piece that ends past n rejects the hit before anything is read.  Then piece j
// must be fold-equal at d over its whole length (piece_at<true>, with its guard against the zero padding behind n: the
// seed guarantees only its own bytes), the candidate (d, j) must stand (edit_side compares the folded text byte with the
// pattern byte; walls as they are), and a piece j' < j that is fold-exact at d and stands there takes the hit.  The
// position the dedupe looks before is d, not di: at() leaves it in m, and edit_scan<true> asks for a standing candidate in
// [start, d).  Each candidate (d, j) has exactly one hit -- the seed of piece j stands at d + its offset in exactly one
// spelling --, so one hit per matching entry survives: the standing candidate with the smallest d and, there, smallest j.
// Bounds and the group-wide-ballot invariant are the exact form's (above, and seed_dedupe_kernel): edit_side judges every
// index before it reads, piece_at checks the piece's end against n first, every tail is masked; before() passes group-wide
// arguments only.  Every loop is bounded by the 4 pieces, by L, by 8 or by 7.  No LDS, no scratch.
template <>
struct EditMatch<true> {
    static constexpr bool kFixedWindow = false;
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32, u32, u32 v, u32 di, u32 &m, u32 plen,
                                              u32 &ls, u32 &ll)
    {
        const u32 budget = T.budget[g], np = budget + 1;
        const u8 *pat = T.bytes + T.off[g];
        const u32 sp = T.pos[v], j = piece_of(sp, plen, np);
        const u32 oj = piece_off(j, plen, np), back = sp - oj;
        if (di < back) return;
        const u32 d = di - back;
        if (!piece_at<true>(ch, d, pat + oj, 0, piece_off(j + 1, plen, np) - oj)) return;     // (false where the piece ends past n)
        bool ok = false;
        for (u32 w = 0; w <= j; ++w) {                            // (at most 4 pieces)
            const u32 off = piece_off(w, plen, np), len = piece_off(w + 1, plen, np) - off;
            if (w < j && !piece_at<true>(ch, d, pat + off, 0, len)) continue;
            const bool st = edit_stands<true>(ch, pat, plen, off, len, d, budget);
            if (w < j && st) break;
            ok = st;
        }
        if (ok) {
            entry_bounds(ch, di, ls, ll);
            m = d;
        }
    }
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32 plen, u32 gl,
                                                  u32 gbase, u32)
    {
        return edit_scan<true>(ch, from, last, T.bytes + T.off[g], plen, nullptr, T.budget[g], gl, gbase);
    }
};
