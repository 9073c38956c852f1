// fold_impl.h -- entries that contain a pattern under ASCII case folding (include/pss.h, pss_reader_search_icase_batch;
// DESIGN.md 4.13).
// Part of search.hip: included there behind sequence_impl.h, whose group geometry (TG lanes per surviving hit) and pair
// spaces it shares, and behind entry_scan_impl.h (fold8, fold_equal, entry_scan); not a header for anybody else.
//
// The suffix arrays are exact-byte, so the host turns every term into its SEED -- the longest window with at most F
// ASCII letters -- and the seed into its 2^f concrete spellings, in ascending byte order (fold_seed and fold_spellings below: what
// pss_icase_variants shows).  A case-insensitive batch has three levels, group -> terms -> spellings, and so three pair
// spaces -- (spelling, chunk), (term, chunk) and (group, chunk); a plain pattern is a group of one include term, an
// all-terms group has its terms, a wildcard pattern its segments.  The spellings of term t are the
// consecutive queries soff[t] .. soff[t + 1]: the interval kernels answer every (spelling, chunk) pair unchanged.  Strings
// of one length in ascending byte order have disjoint, ascending suffix-array intervals, so fold_union_kernel only adds
// the counts up per (term, chunk) pair, and hit k of such a pair is found by walking its at most 64 counts.
// terms_driver_kernel<false> picks every (group, chunk) pair's driver term from those sums.  fold_hits_kernel verifies
// the whole driver term around each of its seed hits under fold and takes the entry's bounds; fold_dedupe_kernel keeps
// the hit of an entry's LEFTMOST folded match: hit_entry's dedupe, under fold (entry_scan<true>).  Every match alignment
// holds exactly one seed occurrence, in exactly one spelling, so an entry keeps exactly one hit whatever mix of spellings
// it holds.  terms_verify_kernel<true> / seq_verify_kernel<true> then check each candidate entry against the group's other
// terms, or its segments in order, under fold.
// A term that holds a 0x0A occurs in no entry and is flagged void: its pairs count no hit.

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

// One lane per (term, chunk) pair: the hits of the pair are the hits of its spellings, one interval behind the other.
// (Disjoint intervals of one suffix array: the sum is at most n and fits u32.)
__global__ __launch_bounds__(256) void fold_union_kernel(u32 nc, const u64 *goff, const u8 *fvoid, const u32 *cnt, u64 ngq, u32 *p_cnt)
{
    const u64 gq = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gq >= ngq) return;
    const u32 g = (u32)(gq / nc), c = (u32)(gq % nc);
    u32 sum = 0;
    if (!fvoid[g])
        for (u32 v = (u32)goff[g], v1 = (u32)goff[g + 1]; v < v1; ++v) sum += cnt[(u64)v * nc + c];
    p_cnt[gq] = sum;
}

// One lane per hit.  The pairs are (group, chunk) pairs and the pattern of pair a is its driver term g_drv[a]; goff
// (the spelling offsets), fseed and foff are indexed by term.  (A pair with hits has a driver that is neither void nor an
// exclude term: terms_driver_kernel.)  Hit k of a pair is suffix sa[lo[v, c] + k'] of the spelling v its walk over the
// driver's counts ends in.  With di that text offset the match would start at m = di - seed_off: out of the chunk ->
// rejected before anything is read.  Else the whole pattern at m under fold (the bytes outside the seed are what is
// unknown; the pattern holds no 0x0A, so a match cannot leave its entry), and the entry's bounds.  A surviving hit leaves
// start, len and m.
__global__ __launch_bounds__(256) void fold_hits_kernel(const ChunkDesc *chunks, u32 nc, const u8 *fbytes, const u64 *foff,
                                                          const u32 *fseed, const u64 *goff, const u32 *lo, const u32 *cnt, u64 ngq,
                                                          const u64 *hit_off, u64 H, u32 *start_out, u32 *len_out, u32 *m_out, const u32 *g_drv)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a], c = (u32)(a % nc);
        const ChunkDesc ch = chunks[c];
        u32 k = (u32)(t - hit_off[a]);
        u32 v = (u32)goff[g];
        const u32 v1 = (u32)goff[g + 1];
        for (; v + 1 < v1; ++v) {                                // (k < the pair's sum: the walk ends inside [goff[g], v1))
            const u32 n_v = cnt[(u64)v * nc + c];
            if (k < n_v) break;
            k -= n_v;
        }
        const u32 di = ch.sa[lo[(u64)v * nc + c] + k];
        const u32 so = fseed[g], plen = (u32)(foff[g + 1] - foff[g]);
        u32 ls = 0, ll = kSkip, m = 0;
        if (di >= so && (u64)(di - so) + plen <= ch.n) {
            m = di - so;
            if (fold_equal(ch.text, m, fbytes + foff[g], plen)) entry_bounds(ch, di, ls, ll);
        }
        start_out[t] = ls;
        len_out[t] = ll;
        m_out[t] = m;
    }
}

// Does a folded occurrence of pat START in text[s, m)?  entry_scan under fold over the start positions s .. m - 1, for
// the TG lanes of one group together.  The match may reach past m: that is safe only because the caller's own match at
// m lies inside the chunk, so every start position p < m has p + plen < n.
__device__ __forceinline__ bool fold_starts_before(const ChunkDesc &ch, u32 s, u32 m, const u8 *pat, u32 plen, u32 gl, u32 gbase)
{
    return m > s && entry_scan<true, false>(ch, s, m - 1, pat, plen, gl, gbase) != kNone;
}

// TG lanes per hit that fold_hits_kernel left standing: the hit is kept iff no folded occurrence of the pattern starts
// in [start, m) -- the leftmost match of the entry stands for it, whichever spelling's interval it came from.  The same
// shape as terms_verify_kernel, for the same reasons: 64 bytes of entry per step, 32 hits per 256-thread workgroup,
// grid-stride.  Every loop is bounded by m - start, an entry's length.  As for fold_hits_kernel, the pattern of pair a
// is its driver term g_drv[a] -- one value per hit, so the group-wide-branch invariant of entry_scan holds.
__global__ __launch_bounds__(256) void fold_dedupe_kernel(const ChunkDesc *chunks, u32 nc, const u8 *fbytes, const u64 *foff, u64 ngq,
                                                            const u64 *hit_off, u64 H, const u32 *start, const u32 *mpos, u32 *len,
                                                            const u32 *g_drv)
{
    const u32 lane = lane_id(), gl = lane & (TG - 1), gbase = lane & ~(TG - 1);
    const u64 step = (u64)gridDim.x * blockDim.x / TG;
    for (u64 t = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / TG; t < H; t += step) {
        if (len[t] == kSkip) continue;
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a];
        const ChunkDesc ch = chunks[(u32)(a % nc)];
        const bool dup = fold_starts_before(ch, start[t], mpos[t], fbytes + foff[g], (u32)(foff[g + 1] - foff[g]), gl, gbase);
        if (dup && gl == 0) len[t] = kSkip;
    }
}
