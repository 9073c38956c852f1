// entry_scan_impl.h -- the one scan of a stretch of an entry for a pattern, by TG lanes together: what the verify kernels
// of all_terms_impl.h and sequence_impl.h and the dedupe of seed_impl.h under fold are built on.
// Part of search.hip: included there behind the entry helpers (cmp_suffix, load_text8, zero_bytes) and in front of the
// files above; not a header for anybody else.

constexpr u32 TG = 8;                            // lanes per candidate entry: 64 bytes per step
constexpr u32 kNone = 0xffffffffu;               // entry_scan: no occurrence

// Bytes of an 8-byte word under fold: 0x20 is set on the bytes in 'A' .. 'Z' and on no other.  Exact per byte, without
// carries between bytes: the low seven bits of a byte plus 0x3f (0x25) set its high bit iff they are >= 0x41 (>= 0x5b),
// and the sums stay below 0x100; a byte >= 0x80 is taken out by its own high bit.
__device__ __forceinline__ u64 fold8(u64 w)
{
    const u64 H = 0x8080808080808080ull;
    const u64 l = w & ~H;
    const u64 ge_a = l + 0x3f3f3f3f3f3f3f3full, gt_z = l + 0x2525252525252525ull;
    return w | ((ge_a & ~gt_z & ~w & H) >> 2);
}

// Is pat (folded, plen bytes) what text[s, s + plen) folds to?  The caller knows s + plen <= n.  Loads reach 15 bytes past
// the last compared byte of the text and 10 past the pattern's end (load_u64_unaligned at the pattern's last byte takes
// three aligned dwords).
__device__ __forceinline__ bool fold_equal(const u8 *text, u32 s, const u8 *pat, u32 plen)
{
    for (u32 i = 0; i < plen; i += 8) {
        u64 a = fold8(load_text8(text + s + i)), b = load_u64_unaligned(pat + i);
        const u32 rem = plen - i;
        if (rem < 8) {
            const u64 mask = (1ull << (8 * rem)) - 1ull;
            a &= mask;
            b &= mask;
        }
        if (a != b) return false;
    }
    return true;
}

// The LEFTMOST start position in from .. last (both inclusive) at which pat (plen >= 1 bytes) stands in the text, or
// kNone.  Fold: the text is compared under ASCII case folding and pat is folded already.  Where = false: the caller only
// asks whether, and any occurrence answers 0 -- the three ballots that read the position out cost terms_verify_kernel
// 0.6 % and fold_dedupe_kernel 2 % when they were compiled in (profiles/entry_scan_refactor.json).  Called by the TG
// lanes of one group together (gl = lane inside the group, gbase = the group's first lane); every lane returns the
// group's answer.
// The caller passes from <= last and knows that a match at `last` ends inside the chunk; a match starts in from .. last
// and nowhere else, so a range that ends plen bytes before an entry's end never reaches the closing newline, the next
// entry or the zero padding behind the chunk.
// All four <Fold, Where> forms are compiled.  <true, true> came last, with entry_find<true> of the case-insensitive
// wildcard search: its ranges end at lim - plen with lim <= n, so the guarantee above holds, and the
// long compare of a candidate at p + k <= last (fold_equal) compares text[p + k, p + k + plen), which ends at or before n.
// Per step the group covers 8 * TG start positions: lane gl takes the 8 that begin at its own 8-byte word, finds the
// bytes equal to the pattern's first byte (zero_bytes) and checks those against the pattern's first min(8, plen) bytes in
// registers -- its word and the one behind it, both folded under Fold; only a pattern longer than 8 bytes whose first 8
// match goes back to memory (cmp_suffix, or fold_equal under Fold).  A lane stops at the LOWEST matching byte of its word
// (the ctz loop ascends), and among the lanes that found one in a step the LOWEST LANE holds the lowest position, since
// lane gl's positions all lie below lane gl + 1's.  Steps ascend too, so the first step with a finding holds the
// leftmost occurrence.
// Loads reach at most 23 bytes past a start position, and under Fold 15 past a match's end (the text is readable 128
// bytes past n, a pattern 16 past its end: 32 zero bytes follow the staged patterns).
template <bool Fold, bool Where>
__device__ __forceinline__ u32 entry_scan(const ChunkDesc &ch, u32 from, u32 last, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    const u64 first = 0x0101010101010101ull * pat[0];
    const u64 pmask = plen >= 8 ? ~0ull : (1ull << (8 * plen)) - 1ull;
    const u64 pk = load_u64_unaligned(pat) & pmask;
    auto rest_equal = [&](u32 s) {                               // the long compare: pat at s, once its first 8 bytes match
        return Fold ? fold_equal(ch.text, s, pat, plen) : cmp_suffix(ch.text, ch.n, s, pat, plen) == 0;
    };
    for (u64 base = from; base <= last; base += 8 * TG) {        // (the same trips for every lane of the group)
        const u64 p64 = base + 8 * gl;
        // What the lane found is kept as a flag, or under Where as the byte of its own word where pat starts (8 = nowhere).
        // The flag form alone takes seq_verify_kernel from 64 to 66 VGPRs, the offset form alone terms_verify_kernel from
        // 95 to 99 SGPRs: a wavefront per SIMD less in either case (profiles/entry_scan_isa.txt).
        bool found = false;
        u32 off = 8;
        if (p64 <= last) {
            const u32 p = (u32)p64;
            u64 w = load_text8(ch.text + p), nxt = load_text8(ch.text + p + 8);
            if (Fold) {
                w = fold8(w);
                nxt = fold8(nxt);
            }
            u64 cand = zero_bytes(w ^ first);
            const u32 nv = last - p + 1;                         // start positions of this word inside the range
            if (nv < 8) cand &= (1ull << (8 * nv)) - 1ull;
            while (cand && (Where ? off == 8 : !found)) {
                const u32 k = (u32)(__builtin_ctzll(cand) >> 3);
                cand &= cand - 1;
                const u64 x = k ? (w >> (8 * k)) | (nxt << (64 - 8 * k)) : w;     // text[p + k, p + k + 8)
                if (Where) {
                    if ((x & pmask) == pk && (plen <= 8 || rest_equal(p + k))) off = k;
                } else if ((x & pmask) == pk)
                    found = plen <= 8 || rest_equal(p + k);
            }
        }
        // The ballots run while the groups of a wavefront are on different paths (other candidates, other patterns, other
        // trip counts); a ballot counts the active lanes only, and only the group's own TG bits are read.  INVARIANT: the
        // TG lanes of a group reach every ballot together -- every branch between the calling kernel's loop entry and a
        // ballot depends on group-wide values only (the hit t and what is read at t, the pair and its group's patterns,
        // earlier answers of this scan, from, last, plen, base, and `who` below, itself a ballot read through the group's
        // bits), and the per-lane `p64 <= last` branch closes above.  A lane that took a path of its own would split the
        // group's ballot, and the lanes would disagree.
        // The winning lane's byte offset reaches the group the same way: three more ballots over the bits of `off`, read at
        // the winner's bit.  (No shuffle: nothing here has to argue that a source lane is active.)
        const u32 who = (u32)(__ballot(Where ? off < 8 : found) >> gbase) & ((1u << TG) - 1u);
        if (who) {
            if (!Where) return 0;
            const u32 wl = (u32)__builtin_ctz(who);              // the lowest lane that found one
            const u32 b0 = (u32)(__ballot((off & 1u) != 0) >> (gbase + wl)) & 1u;
            const u32 b1 = (u32)(__ballot((off & 2u) != 0) >> (gbase + wl)) & 1u;
            const u32 b2 = (u32)(__ballot((off & 4u) != 0) >> (gbase + wl)) & 1u;
            return (u32)base + 8 * wl + (b0 | (b1 << 1) | (b2 << 2));
        }
    }
    return kNone;
}
