// any_impl.h -- entries that hold at least one of a set of alternatives (include/pss.h, pss_reader_search_any_batch;
// DESIGN.md 4.22).
// Part of search.hip: included there behind fold_impl.h and seed_impl.h, whose seeded verify path it gives the compare of
// a SET, and behind entry_scan_impl.h (fold_equal, entry_scan); not a header for anybody else.
//
// The host normalises every set (any_terms.h): folded to lower case under fold, no duplicate, no alternative with a 0x0A,
// none that holds another as a substring, ascending.  What is left is PREFIX-FREE -- no two alternatives can start at one
// text position -- and is the set's one term, its alternatives back to back.  Its seed queries are, exact: the alternatives
// themselves, each at position 0; under fold: alternative by alternative the spellings of its seed, each at the seed's
// position inside the ALTERNATIVE.  A query belongs to an alternative, not to the term: AnyAlts (seed_impl.h) says which,
// and where the alternatives lie.  Exact alternatives, ascending and prefix-free, have disjoint ascending intervals; under
// fold two alternatives may share a seed (`ab1234`, `cb1234` at one letter), so a pair's sum can pass n and the batch
// hands seed_union_kernel the overflow word, as a near batch does.
//
// One hit per matching entry.  The leftmost position of the entry at which any alternative stands is one position, and
// one alternative stands there (prefix-free); under fold one spelling of that alternative's seed stands at its offset
// behind it.  So exactly one query has a hit whose window starts there: AnyMatch::at lets every hit stand whose alternative
// stands around it, AnyMatch::before drops those with a start of ANY alternative of the set in front of them.
//
// Bounds.  any_request_ok (search_layout.h) has held every query's alternative j to its term's alternatives, every
// alternative to a non-empty stretch of the term's bytes, and pos + the query's length to the alternative's length.
// at: the window is [w, w + len_j) with w = di - pos; di < pos and w + len_j > n are rejected before anything is read, so
// fold_equal compares inside [0, n) (its loads: 15 bytes past the window, 10 past the alternative -- the text is readable
// 128 bytes past n, 32 zero bytes follow the terms; the tail is masked, so a 0x00 at an alternative's end is not taken
// as equal to that padding).  Exact bytes need no compare: the query is the alternative, and the suffix array found it.
// before: the lengths differ, so "a window in front of m ends before m + L <= n" no longer holds -- a 40-byte alternative
// that starts one byte before a 2-byte match at the end of an unterminated chunk would be compared past n + 128.  So
// alternative j is scanned over [start, min(m - 1, end - len_j)] with `end` the entry's true end (the closing newline, or
// n for an unterminated last entry, told apart as regex_verify_kernel does), and skipped where that range is empty: a
// match at the range's last position ends at or before end <= n, which is what entry_scan asks of its caller, and it
// cannot lie elsewhere -- an alternative holds no 0x0A and so never leaves the entry.  The loop runs over the term's
// alternatives, at most 64; the scan's loops are bounded by an entry's length.  Writes: none of its own (the two kernels
// write start[t], len[t], m[t] of their own hit).  No LDS, no scratch.

template <bool Fold>
struct AnyMatch {
    static constexpr bool kFixedWindow = false;     // the term's length means nothing: the frame passes di through, `at` rejects
    // The alternative of query v around di: under fold over its whole length (the seed vouches for its own bytes only), then
    // the entry's bounds.  Leaves the alternative's start in m for the dedupe.
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32, u32, u32, u32 v, u32 di, u32 &m, u32, u32 &ls,
                                              u32 &ll)
    {
        const AnyAlts A = *T.any;
        const u32 j = A.qalt[v], pos = T.pos[v];
        const u64 a0 = A.aoff[j];
        const u32 alen = (u32)(A.aoff[j + 1] - a0);
        if (di < pos || (u64)(di - pos) + alen > ch.n) return;
        const u32 w = di - pos;
        if (Fold && !fold_equal(ch.text, w, T.bytes + a0, alen)) return;
        entry_bounds(ch, di, ls, ll);
        m = w;
    }
    // Does any alternative of term g START in text[from, last]?  from = the entry's start, elen its length as entry_bounds
    // left it.  INVARIANT (seed_dedupe_kernel's): the TG lanes of a group reach every ballot of entry_scan together -- the
    // trip count is the term's number of alternatives, `end`, every alternative's length and range and the answer of an
    // earlier scan (itself a ballot) are the same for the group's lanes; nothing here depends on gl.
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32, u32 gl, u32 gbase,
                                                  u32 elen)
    {
        const AnyAlts A = *T.any;
        const u32 e = from + elen;                               // e <= n - 1: the closing newline, or the last byte
        const u32 end = ch.text[e] == '\n' ? e : ch.n;
        const u32 j1 = (u32)A.talts[g + 1];
        for (u32 j = (u32)A.talts[g]; j < j1; ++j) {
            const u64 a0 = A.aoff[j];
            const u32 alen = (u32)(A.aoff[j + 1] - a0);
            if (end - from < alen) continue;                     // (longer than the entry)
            const u32 hi = last < end - alen ? last : end - alen;
            if (entry_scan<Fold, false>(ch, from, hi, T.bytes + a0, alen, gl, gbase) != kNone) return true;
        }
        return false;
    }
};
