// anchored_impl.h -- anchored search: entries that START WITH, END WITH or EQUAL a pattern (include/pss.h,
// pss_reader_search_anchored_batch).
// Part of search.hip: included there behind the entry helpers (cmp_suffix, entry_bounds) and the workspace slots; not a
// header for anybody else.
//
// Every entry but the first of a chunk has a 0x0A before it and every entry but an unterminated last one has a 0x0A
// behind it, so the entries that start with `pat` are the hits of "\n" + pat, the ones that end with it the hits of
// pat + "\n" and the ones equal to it the hits of "\n" + pat + "\n": the host rewrites the queries, the interval
// kernels of search.hip run on them unchanged, and the interval holds ONE hit per matching entry -- no dedupe, no
// backward scan for an earlier match.  What the interval cannot hold are the two entries at the ends of the chunk:
//   head  the entry at offset 0 (no newline before it),
//   tail  the last entry of a text that does not end in a newline (none behind it).
// anchor_edges_kernel tests those two per (query, chunk) pair and adds them to the pair's hit count, so the scans
// size everything as always; anchored_hits_kernel turns hit t of a pair -- interval hits first, then the head, then
// the tail -- into the bounds of its entry.  From there the pipeline is the general one of search_batch_device.
// A pattern that holds a 0x0A matches nothing (an entry never holds one), but its rewritten form could hit: such a
// query is flagged on the host and its pairs count zero hits.

constexpr u8 kAnchorStart = PSS_ANCHOR_START, kAnchorEnd = PSS_ANCHOR_END;
constexpr u8 kAnchorVoid = 0x80;                 // the pattern holds a newline: no hit
constexpr u8 kEdgeHead = 1, kEdgeTail = 2;       // per pair: which chunk-edge hits follow the interval hits

// Bytes of the rewritten queries of a batch.
static u64 anchored_query_bytes(const u64 *qoff, u32 nq, const u8 *anchors)
{
    u64 total = qoff[nq];
    for (u32 q = 0; q < nq; ++q) total += ((anchors[q] & kAnchorStart) ? 1u : 0u) + ((anchors[q] & kAnchorEnd) ? 1u : 0u);
    return total;
}

// The rewritten queries, their offsets (nq + 1) and the per-query flags (nq); 32 zero bytes behind the queries as
// everywhere (the kernels read past a query's end).
static void anchored_rewrite(const u8 *qbytes, const u64 *qoff, u32 nq, const u8 *anchors, u8 *out, u64 *out_off, u8 *flags)
{
    u64 at = 0;
    newline_flags(qbytes, qoff, nq, kAnchorVoid, flags);
    for (u32 q = 0; q < nq; ++q) {
        const u8 *pat = qbytes + qoff[q];
        const u64 m = qoff[q + 1] - qoff[q];
        out_off[q] = at;
        if (anchors[q] & kAnchorStart) out[at++] = '\n';
        if (m) memcpy(out + at, pat, m);
        at += m;
        if (anchors[q] & kAnchorEnd) out[at++] = '\n';
        flags[q] |= anchors[q];
    }
    out_off[nq] = at;
    memset(out + at, 0, 32);
}

// One lane per (query, chunk) pair: the head and the tail of the chunk against the pattern (the rewritten query
// without its newlines).  cnt[vq] comes in as the interval's hits and leaves as the pair's hits.
__global__ __launch_bounds__(256) void anchor_edges_kernel(const ChunkDesc *chunks, u32 nc, const u8 *qbytes, const u64 *qoff,
                                                             const u8 *flags, u64 nvq, u32 *cnt, u8 *edge)
{
    const u64 vq = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (vq >= nvq) return;
    const u32 q = (u32)(vq / nc), c = (u32)(vq % nc);
    const u8 f = flags[q];
    if (f & kAnchorVoid) {
        cnt[vq] = 0;
        edge[vq] = 0;
        return;
    }
    const bool at_start = (f & kAnchorStart) != 0, at_end = (f & kAnchorEnd) != 0;
    const u8 *pat = qbytes + qoff[q] + (at_start ? 1 : 0);
    const u32 m = (u32)(qoff[q + 1] - qoff[q]) - (at_start ? 1u : 0u) - (at_end ? 1u : 0u);
    const ChunkDesc ch = chunks[c];
    const u32 n = ch.n;
    u8 e = 0;
    if (n && m <= n) {
        // head: text[0, m) == pat; an exact match also ends there (m == n is the whole chunk)
        if (at_start && cmp_suffix(ch.text, n, 0, pat, m) == 0 && (!at_end || m == n || ch.text[m] == '\n')) e |= kEdgeHead;
        // tail: no newline closes the text and text[n - m, n) == pat; an exact match also starts there (n == m was the head's)
        if (at_end && ch.text[n - 1] != '\n' && cmp_suffix(ch.text, n, n - m, pat, m) == 0 &&
            (!at_start || (n > m && ch.text[n - m - 1] == '\n')))
            e |= kEdgeTail;
    }
    edge[vq] = e;
    cnt[vq] += (u32)__popc((u32)e);
}

// hit_lines_kernel of the anchored search: one thread per hit, the bounds of its entry.  Interval hit k of the pair is
// the suffix sa[lo + k], which starts at the newline BEFORE the entry when the query was given one; the head lies at
// offset 0, the tail around n - 1.  Every hit is another entry, so every hit is kept -- but one: "\n" alone (the empty
// pattern anchored at the start) also hits the chunk's closing newline, behind which no entry starts.
__global__ __launch_bounds__(256) void anchored_hits_kernel(const ChunkDesc *chunks, u32 nc, const u8 *flags, u64 nvq, const u32 *lo,
                                                              const u8 *edge, const u64 *hit_off, u64 H, u32 *start_out, u32 *len_out)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        const u64 a = pair_of_hit(hit_off, nvq, t);
        const ChunkDesc ch = chunks[(u32)(a % nc)];
        const u8 f = flags[a / nc], e = edge[a];
        const u32 k = (u32)(t - hit_off[a]);
        const u32 in_interval = (u32)(hit_off[a + 1] - hit_off[a]) - (u32)__popc((u32)e);
        u32 di;
        if (k < in_interval) di = ch.sa[lo[a] + k] + ((f & kAnchorStart) ? 1u : 0u);
        else if (k == in_interval && (e & kEdgeHead)) di = 0;
        else di = ch.n - 1;
        if (di >= ch.n) {
            start_out[t] = 0;
            len_out[t] = kSkip;
            continue;
        }
        u32 ls = 0, ll = 0;
        entry_bounds(ch, di, ls, ll);
        start_out[t] = ls;
        len_out[t] = ll;
    }
}
