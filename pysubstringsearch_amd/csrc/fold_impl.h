// fold_impl.h -- entries that contain a pattern under ASCII case folding (include/pss.h, pss_reader_search_icase_batch;
// DESIGN.md 4.13, 4.14).
// Part of search.hip: included there behind seed_impl.h, whose seeded verify path it gives the compare under fold, and
// behind entry_scan_impl.h (fold8, fold_equal, entry_scan); not a header for anybody else.
//
// The suffix arrays are exact-byte, so the host turns every term into its SEED -- the longest window with at most F
// ASCII letters -- and the seed into its 2^f concrete spellings, in ascending byte order (fold_seed and fold_spellings below: what
// pss_icase_variants shows).  The spellings are the seed queries of the term (seed_impl.h), every one at the seed's offset
// inside it; a plain pattern is a group of one include term, an all-terms group has its terms, a wildcard pattern its
// segments.  Strings of one length in ascending byte order have disjoint, ascending suffix-array
// intervals, so a (term, chunk) pair's sum is at most n, and every match alignment holds exactly one seed occurrence, in
// exactly one spelling: an entry keeps exactly one hit whatever mix of spellings it holds.  After the two seeded kernels,
// terms_verify_kernel<true> / seq_verify_kernel<true> check each candidate entry against the group's other terms, or its
// segments in order, under fold.

// The seed of pat[0, len): the longest window with at most `letters` ASCII letters, the leftmost on a tie.  Returns its
// letter count.  (Host code, declared in search.h: the C ABI expands the patterns before it states the request.)
u32 fold_seed(const u8 *pat, u64 len, u32 letters, u64 *seed_off, u64 *seed_len)
{
    auto is_letter = [](u8 b) { return (u8)((b | 0x20u) - 'a') < 26u; };
    u64 best_off = 0, best_len = 0, i = 0;
    u32 in_window = 0, best_letters = 0;
    for (u64 j = 0; j < len; ++j) {              // [i, j]: the longest window that ends at j
        in_window += is_letter(pat[j]) ? 1u : 0u;
        while (in_window > letters) in_window -= is_letter(pat[i++]) ? 1u : 0u;
        if (j + 1 - i > best_len) {
            best_len = j + 1 - i;
            best_off = i;
            best_letters = in_window;
        }
    }
    *seed_off = best_off;
    *seed_len = best_len;
    return best_letters;
}

// The 2^f spellings of seed[0, len) (f letters) back to back into out, ascending bytewise: upper case sorts before lower,
// and the first letter is the most significant.
void fold_spellings(const u8 *seed, u64 len, u32 f, u8 *out)
{
    for (u32 v = 0; v < (1u << f); ++v) {
        u32 bit = f;
        for (u64 i = 0; i < len; ++i) {
            u8 b = seed[i];
            if ((u8)((b | 0x20u) - 'a') < 26u) b = (v >> --bit) & 1u ? (u8)(b | 0x20u) : (u8)(b & ~0x20u);
            out[(u64)v * len + i] = b;
        }
    }
}

// The compare of the seeded path (seed_impl.h) under fold; the terms are folded to lower case already.
struct FoldMatch {
    static constexpr bool kFixedWindow = true;      // the term stands at m = di - pos or not at all: the frame rejects a window that leaves the chunk
    // The whole term at m under fold (the bytes outside the seed are what is unknown; the term holds no 0x0A, so a match
    // cannot leave its entry), then the entry's bounds.
    static __device__ __forceinline__ void at(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32, u32, u32, u32 di, u32 &m, u32 plen,
                                              u32 &ls, u32 &ll)
    {
        if (fold_equal(ch.text, m, T.bytes + T.off[g], plen)) entry_bounds(ch, di, ls, ll);
    }
    // Does a folded occurrence of the term START in text[from, last]?  entry_scan under fold, for the TG lanes of one
    // group together.
    static __device__ __forceinline__ bool before(const ChunkDesc &ch, const SeedTerms &T, u32 g, u32 from, u32 last, u32 plen, u32 gl,
                                                  u32 gbase, u32)
    {
        return entry_scan<true, false>(ch, from, last, T.bytes + T.off[g], plen, gl, gbase) != kNone;
    }
};
