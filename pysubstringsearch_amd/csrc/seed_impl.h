// seed_impl.h -- the one seeded verify path of the case-insensitive search (fold_impl.h) and of the search within k
// mismatches (near_impl.h): DESIGN.md 4.16.
// Part of search.hip: included there behind entry_scan_impl.h (TG, the group geometry) and the entry helpers
// (pair_of_hit, entry_bounds), in front of fold_impl.h and near_impl.h, which state the two compares; not a header for
// anybody else.
//
// A TERM is a whole pattern as it is verified.  The suffix arrays answer exact queries only, so the host looks a term up
// through several exact SEED QUERIES, each standing at a known position inside the term: the spellings of its seed (fold)
// or its k + 1 pieces (near).  A seeded batch has three levels, group -> terms -> seed queries, and so three pair spaces:
// (query, chunk), what the interval kernels answer unchanged; (term, chunk), what seed_union_kernel adds the counts up to;
// (group, chunk), what terms_driver_kernel<false> picks a driver term for and everything from the first scan on runs
// over.  The queries of term g are the consecutive queries soff[g] .. soff[g + 1]; hit k of a (term, chunk) pair is found
// by walking the counts of those queries.  With di the text offset of a seed hit and pos the position of its query
// inside the term, the term would start at m = di - pos: seed_hits_kernel verifies the whole term there (Match::at) and
// seed_dedupe_kernel keeps the hit of the entry's LEFTMOST match (Match::before).  What "the term stands at m" means is
// the Match's: FoldMatch compares under ASCII case folding, NearMatch exact bytes within a budget of mismatches.  A third,
// EditMatch (edit_impl.h), allows insertions and deletions too: it has no fixed window, so for it m is di
// itself, Match::at asks whether the CANDIDATE (piece, di) stands and Match::before whether one stands in front of di.
// A fourth, AnyMatch (any_impl.h), takes a term that is a SET of alternatives back to back: a query belongs
// to one alternative, Match::at verifies that one where the query's position puts it and Match::before asks whether ANY
// alternative starts in front of it -- windows of several lengths, which is why before() is handed the entry's length.
// A term that holds a 0x0A occurs in no entry and is flagged void: its pairs count no hit.
//
// Bounds, for both kernels and the two kinds with a fixed window (edit_impl.h states its own: it walks byte by byte and
// stops at the entry's ends).  A window that is read lies in [0, n): seed_hits_kernel rejects di < pos and
// m + L > n before anything is read, and every window the dedupe looks at starts before m and so ends before m + L <= n.
// Text loads are load_text8 at a byte of such a window or 8 past a start position: at most 23 bytes past a start position
// and 15 past a compared range (the text is readable 128 bytes past n).  A term is read by load_u64_unaligned at one of
// its bytes: at most 10 bytes past its end (32 zero bytes follow the terms on the device).  The tail of every compare is
// masked, so a 0x00 at a term's end is never taken as equal to that padding, nor a text byte behind the window as part of
// it.  The two kernels write start[t], len[t], m[t] of their own hit t and nothing else.  No LDS, no scratch.

// The terms of a seeded batch on the device (Batch::seed_drivers): bytes / off are the terms back to back and their
// nterms + 1 offsets, soff the nterms + 1 offsets into the queries, pos the position of every QUERY inside its term,
// budget the mismatches allowed per term -- null under fold.
// An any-of batch (any_impl.h) has no budgets and puts its own block in their place: `any` points at the
// three pointers of AnyAlts on the device (AnyBlock of search_layout.h), so that SeedTerms keeps its size and every kernel
// its arguments.
struct AnyAlts {
    const u64 *talts;       // nterms + 1: the alternatives of term g are talts[g] .. talts[g + 1]
    const u64 *aoff;        // alternatives + 1: alternative j is bytes[aoff[j], aoff[j + 1])
    const u32 *qalt;        // per query: the alternative it was taken from (pos[v] is its position inside THAT)
};
struct SeedTerms {
    const u8 *bytes;
    const u64 *off;
    const u64 *soff;
    const u32 *pos;
    union {
        const u8 *budget;
        const AnyAlts *any;
    };
};

// One lane per (term, chunk) pair: the hits of the pair are the hits of its queries, one interval behind the other.
// The spellings of a seed have disjoint intervals (strings of one length), so their sum is at most n; the pieces of a
// pattern may overlap, nest or repeat, so theirs can reach (k + 1) n.  The sum is taken in 64 bits, and THIS is where a
// pair of more than 2^32 - 1 hits is caught: the pair counts 0 and raises *over, which fails the batch on the host before
// any hit buffer is reserved (Batch::run_general).  over = null: the caller knows the sum fits (a fold batch).  The flag
// takes a chunk of more than 2^30 bytes of one piece: out of a test's reach, checked by reading.
__global__ __launch_bounds__(256) void seed_union_kernel(u32 nc, const u64 *soff, const u8 *fvoid, const u32 *cnt, u64 ngq, u32 *p_cnt,
                                                           u64 *over)
{
    const u64 gq = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gq >= ngq) return;
    const u32 g = (u32)(gq / nc), c = (u32)(gq % nc);
    u64 sum = 0;
    if (!fvoid[g]) {
        u32 v = (u32)soff[g];
        const u32 v1 = (u32)soff[g + 1];
        for (; v + 4 <= v1; v += 4) {           // (four loads in flight: up to 64 spellings, and one load a trip waits for each)
            const u32 a = cnt[(u64)v * nc + c], b = cnt[(u64)(v + 1) * nc + c], d = cnt[(u64)(v + 2) * nc + c], e = cnt[(u64)(v + 3) * nc + c];
            sum += (u64)a + b + d + e;
        }
        for (; v < v1; ++v) sum += cnt[(u64)v * nc + c];
    }
    if (sum > 0xffffffffull) {
        if (over) *over = 1;
        sum = 0;
    }
    p_cnt[gq] = (u32)sum;
}

// One lane per hit.  The pairs are (group, chunk) pairs and the term of pair a is its driver term g_drv[a].  (A pair with
// hits has a driver that is neither void nor an exclude term: terms_driver_kernel.)  Hit k of a pair is suffix
// sa[lo[v, c] + k'] of the query v its walk over the driver's counts ends in.  With di that text offset the term would
// start at m = di - pos[v]: out of the chunk -> rejected before anything is read.  Else Match::at says whether the term
// stands at m and, where it does, leaves the bounds of the entry around di in ls / ll.  A surviving hit leaves start, len
// and m.  That reject is right for a Match with a FIXED WINDOW (Match::kFixedWindow: fold, near).  Under edits
// (EditMatch) it is wrong -- a deletion left of the piece lets the match start behind di - pos, one right of it lets it
// end before di - pos + L, so a match flush with the chunk's start or end would be lost --: there the frame passes di
// through, m is di itself, and what m_out[t] means is "the position the dedupe looks before".  Match::at takes m by
// reference: a Match whose candidate does not stand where its query was found (EditMatch<true>, DESIGN.md 4.19: the query
// is the seed of a piece) leaves the candidate's position there; every other Match leaves m alone.
template <typename Match>
__global__ __launch_bounds__(256) void seed_hits_kernel(const ChunkDesc *chunks, u32 nc, SeedTerms T, const u32 *lo, const u32 *cnt, u64 ngq,
                                                          const u64 *hit_off, u64 H, u32 *start_out, u32 *len_out, u32 *m_out, const u32 *g_drv)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a], c = (u32)(a % nc);
        const ChunkDesc ch = chunks[c];
        u32 k = (u32)(t - hit_off[a]);
        const u32 v0 = (u32)T.soff[g], v1 = (u32)T.soff[g + 1];
        u32 v = v0;
        for (; v + 1 < v1; ++v) {                                // (k < the pair's sum: the walk ends inside [v0, v1))
            const u32 n_v = cnt[(u64)v * nc + c];
            if (k < n_v) break;
            k -= n_v;
        }
        const u32 di = ch.sa[lo[(u64)v * nc + c] + k];
        const u32 pos = T.pos[v], plen = (u32)(T.off[g + 1] - T.off[g]);
        u32 ls = 0, ll = kSkip, m = 0;
        if (!Match::kFixedWindow || (di >= pos && (u64)(di - pos) + plen <= ch.n)) {
            m = Match::kFixedWindow ? di - pos : di;
            Match::at(ch, T, g, v0, v1, v, di, m, plen, ls, ll);
        }
        start_out[t] = ls;
        len_out[t] = ll;
        m_out[t] = m;
    }
}

// TG lanes per hit that seed_hits_kernel left standing: the hit is kept iff no match of the term STARTS in [start, m)
// (Match::before) -- the leftmost match of the entry stands for it, whichever query's interval it came from.  Such a match
// may reach past m; it ends before m + L, hence inside the chunk.  The same shape as terms_verify_kernel, for the same
// reasons: 64 bytes of entry per step, 32 hits per 256-thread workgroup, grid-stride.  Every loop is bounded by
// m - start, an entry's length.
// INVARIANT (entry_scan's, restated once for both scans): the TG lanes of a group reach every ballot of Match::before
// together.  Every branch between the loop entry and those ballots depends on t, on what is read at t (len, start, m) and
// on the pair's term -- one driver g_drv[a] per hit -- and never on gl.  (m <= s is judged before the pair is looked up:
// behind it the loads of the driver and of its offsets would wait for that branch, one after the other.)
template <typename Match>
__global__ __launch_bounds__(256) void seed_dedupe_kernel(const ChunkDesc *chunks, u32 nc, SeedTerms T, u64 ngq, const u64 *hit_off, u64 H,
                                                            const u32 *start, const u32 *mpos, u32 *len, const u32 *g_drv)
{
    const u32 lane = lane_id(), gl = lane & (TG - 1), gbase = lane & ~(TG - 1);
    const u64 step = (u64)gridDim.x * blockDim.x / TG;
    for (u64 t = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / TG; t < H; t += step) {
        const u32 l = len[t];
        if (l == kSkip) continue;
        const u32 s = start[t], m = mpos[t];
        if (m <= s) continue;                                    // (the match stands at the entry's start: nothing starts before it)
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = g_drv[a];
        const ChunkDesc ch = chunks[(u32)(a % nc)];
        // (l, the entry's length as entry_bounds left it: AnyMatch alone asks for it -- its windows have several lengths)
        const bool dup = Match::before(ch, T, g, s, m - 1, (u32)(T.off[g + 1] - T.off[g]), gl, gbase, l);
        if (dup && gl == 0) len[t] = kSkip;
    }
}
