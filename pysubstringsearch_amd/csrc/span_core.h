// span_core.h -- match spans: how one START POSITION of an entry scores against a pattern, and the key that orders the
// scores (include/pss.h, pss_reader_match_spans).
// Plain C++ that compiles inside search.hip (span_impl.h: one lane per start position) and under g++ alone
// (tests/native/span_core.cpp: the same functions start by start under AddressSanitizer).  It calls into neither
// near_impl.h nor edit_impl.h, which are device code: the word compare and the band below restate theirs.
//
// A row's answer is the candidate e[s : s + l] with the least (d, s, -l), d its distance within the budget k <= 3.  One
// start s has at most one candidate worth keeping -- without edits the window of L bytes, with edits the longest of the
// lengths L - 3 .. L + 3 that reach the start's least distance -- and its key is
//   d << 35 | s << 3 | (L + 3 - l)
// so that the unsigned minimum over the starts is the answer: d <= 3, s < 2^32, L + 3 - l = 0 .. 6.  kSpanNone (all ones)
// is "no candidate here" and loses to every key.
//
// Bounds.  span_mismatches reads text[at + i, at + i + 8) and pat[i, i + 8) for i = 0, 8, .. < L of a window the caller
// knows to end at or before the entry's end (<= n): at most 7 bytes past the window and past the pattern, tails masked
// (the text is readable 128 bytes past n; kSpanPatPad zero bytes follow the patterns).  span_edit_key is edit_side's
// walk: one text byte at a time at an index it has judged to lie in [at, n), stopping for good at the first 0x0A or at
// n, so the zero padding is never taken for text and nothing below `at` is read; the pattern one byte at a time inside
// [0, L).  No LDS, no scratch: the band and its text window are named registers.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIP__)
#define PSS_HD __host__ __device__ __forceinline__
#else
#define PSS_HD inline
#endif

namespace pss {

constexpr uint32_t kSpanMaxBudget = 3;                  // (kNearMaxBudget: the band below holds 2 * 3 + 1 columns)
constexpr uint64_t kSpanNone = ~0ull;
constexpr uint32_t kSpanPatPad = 8;                     // zero bytes behind the uploaded patterns
constexpr uint32_t kSpanInf = 64;                       // above every budget and every cell that counts
constexpr uint32_t kSpanWall = 0x100;                   // (no byte: the entry ends here)
constexpr uint32_t kSpanNoByte = 0x200;                 // (no byte: in front of the start)

PSS_HD uint64_t span_key(uint32_t d, uint32_t s, uint32_t L, uint32_t l)
{
    return (uint64_t)d << 35 | (uint64_t)s << 3 | (uint64_t)(L + 3 - l);
}

// (start, length, distance) of a key; (-1, 0, -1) of kSpanNone.
PSS_HD void span_unkey(uint64_t key, uint32_t L, int32_t *out)
{
    const bool none = key == kSpanNone;
    out[0] = none ? -1 : (int32_t)(uint32_t)(key >> 3);
    out[1] = none ? 0 : (int32_t)(L + 3 - (uint32_t)(key & 7));
    out[2] = none ? -1 : (int32_t)(key >> 35);
}

PSS_HD uint64_t span_load8(const uint8_t *p)
{
    uint64_t w;
    memcpy(&w, p, 8);
    return w;
}

// A-Z of every byte of w to a-z, nothing else (no cross-byte carries: the sums stay below 0x100 per byte).
PSS_HD uint64_t span_fold8(uint64_t w)
{
    const uint64_t low = w & 0x7f7f7f7f7f7f7f7full;
    const uint64_t ge_a = low + 0x3f3f3f3f3f3f3f3full, gt_z = low + 0x2525252525252525ull;
    return w | ((ge_a & ~gt_z & ~w & 0x8080808080808080ull) >> 2);
}

PSS_HD uint32_t span_nonzero_bytes(uint64_t x)
{
    const uint64_t m = 0x7f7f7f7f7f7f7f7full;
    return (uint32_t)__builtin_popcountll((((x & m) + m) | x) & ~m);
}

// Mismatches of pat[0, L) against text[at, at + L); gives up -- with a value above `budget` -- as soon as the budget is
// exceeded.  kFold: the text word is folded before the xor (pat is folded already).
template <bool kFold>
PSS_HD uint32_t span_mismatches(const uint8_t *text, uint32_t at, const uint8_t *pat, uint32_t L, uint32_t budget)
{
    uint32_t have = 0;
    for (uint32_t i = 0; i < L && have <= budget; i += 8) {
        const uint64_t tw = span_load8(text + at + i);
        uint64_t x = (kFold ? span_fold8(tw) : tw) ^ span_load8(pat + i);
        const uint32_t rem = L - i;
        if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;
        have += span_nonzero_bytes(x);
    }
    return have;
}

// The window of L bytes at start s of the entry text[es, es + elen): its key, or kSpanNone when it leaves the entry or
// differs in more than `budget` bytes.
template <bool kFold>
PSS_HD uint64_t span_window_key(const uint8_t *text, uint32_t es, uint32_t elen, uint32_t s, const uint8_t *pat, uint32_t L, uint32_t budget)
{
    if (elen < L || s > elen - L) return kSpanNone;
    const uint32_t d = span_mismatches<kFold>(text, es + s, pat, L, budget);
    return d <= budget ? span_key(d, s, L, L) : kSpanNone;
}

PSS_HD uint32_t span_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// One cell of the band (edit_impl.h, edit_cell): D[i][t] from its three neighbours, w the text byte of column t, pc the
// pattern byte of row i.  A column at or behind a wall does not exist; a value above the budget can only grow.
PSS_HD uint32_t span_cell(uint32_t left, uint32_t diag, uint32_t up, uint32_t w, uint32_t pc, uint32_t budget)
{
    uint32_t v = diag + (w != pc ? 1u : 0u);
    v = span_min(v, span_min(up, left) + 1u);
    return (w == kSpanWall || v > budget) ? kSpanInf : v;
}

// Start s of the entry that begins at text[es] (at = es + s < n, the text of a chunk of n bytes): the least
// d = lev(text[at, at + l), pat) over l, and the LARGEST l that reaches it, as a key; kSpanNone when d > budget.
// edit_side<false, kFold>'s band walked to its last row, whose cells r0 .. r6 are the lengths l = L - 3 .. L + 3 (a
// length below 1 holds a value above the budget, since L > budget).  The walk ends at the entry's newline or at n by
// itself: it needs no entry length.  At most L trips of 7 cells.
template <bool kFold>
PSS_HD uint64_t span_edit_key(const uint8_t *text, uint32_t n, uint32_t at, uint32_t s, const uint8_t *pat, uint32_t L, uint32_t budget)
{
    uint32_t taken = 0;
    bool wall = false;
    // The next byte of the entry, or a wall; a wall stays a wall.  The index is judged first; a lane that stands at a wall
    // loads text[at] again (at < n) and drops what it loaded.
    auto next = [&]() -> uint32_t {
        const bool in = !wall && (uint64_t)at + taken < n;
        const uint32_t b0 = text[in ? at + taken : at];
        const uint32_t b = kFold && b0 - 'A' < 26u ? b0 | 0x20u : b0;
        wall = !in || b == '\n';
        taken += wall ? 0u : 1u;
        return wall ? kSpanWall : b;
    };
    uint32_t w0 = kSpanNoByte, w1 = kSpanNoByte, w2 = kSpanNoByte, w3 = next(), w4 = next(), w5 = next(), w6 = next();
    uint32_t r0 = kSpanInf, r1 = kSpanInf, r2 = kSpanInf, r3 = 0;
    uint32_t r4 = (w3 != kSpanWall && budget >= 1) ? 1u : kSpanInf;
    uint32_t r5 = (w4 != kSpanWall && budget >= 2) ? 2u : kSpanInf;
    uint32_t r6 = (w5 != kSpanWall && budget >= 3) ? 3u : kSpanInf;
    for (uint32_t i = 1; i <= L; ++i) {
        if (i > 1) {
            w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6;
            w6 = next();
        }
        const uint32_t pc = pat[i - 1];
        const uint32_t c0 = span_cell(kSpanInf, r0, r1, w0, pc, budget);
        const uint32_t c1 = span_cell(c0, r1, r2, w1, pc, budget);
        const uint32_t c2 = span_cell(c1, r2, r3, w2, pc, budget);
        const uint32_t c3 = span_cell(c2, r3, r4, w3, pc, budget);
        const uint32_t c4 = span_cell(c3, r4, r5, w4, pc, budget);
        const uint32_t c5 = span_cell(c4, r5, r6, w5, pc, budget);
        const uint32_t c6 = span_cell(c5, r6, kSpanInf, w6, pc, budget);
        r0 = c0; r1 = c1; r2 = c2; r3 = c3; r4 = c4; r5 = c5; r6 = c6;
        if (span_min(span_min(span_min(r0, r1), span_min(r2, r3)), span_min(span_min(r4, r5), r6)) > budget) return kSpanNone;
    }
    uint32_t d = r0, j = 0;                             // the largest column among the least values
    if (r1 <= d) { d = r1; j = 1; }
    if (r2 <= d) { d = r2; j = 2; }
    if (r3 <= d) { d = r3; j = 3; }
    if (r4 <= d) { d = r4; j = 4; }
    if (r5 <= d) { d = r5; j = 5; }
    if (r6 <= d) { d = r6; j = 6; }
    return d <= budget ? span_key(d, s, L, L - 3 + j) : kSpanNone;
}

// What lane `s` of a step computes: the key of start s of the entry text[es, es + elen) of a chunk of n bytes.
template <bool kFold, bool kEdits>
PSS_HD uint64_t span_start_key(const uint8_t *text, uint32_t n, uint32_t es, uint32_t elen, uint32_t s, const uint8_t *pat, uint32_t L,
                               uint32_t budget)
{
    if (kEdits) return s < elen ? span_edit_key<kFold>(text, n, es + s, s, pat, L, budget) : kSpanNone;
    return span_window_key<kFold>(text, es, elen, s, pat, L, budget);
}

// Start positions a row walks, 64 a step: every window that fits, or every byte of the entry.
PSS_HD uint32_t span_starts(uint32_t elen, uint32_t L, bool edits)
{
    return edits ? elen : (elen >= L ? elen - L + 1 : 0u);
}

}  // namespace pss
