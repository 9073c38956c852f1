// regex_impl.h -- the verify step of the regular-expression search (include/pss.h, pss_reader_search_regex_batch;
// DESIGN.md 4.21).  Part of search.hip: included there behind all_terms_impl.h, whose candidates it takes; not a header
// for anybody else.
//
// A regex batch is an all-terms batch over the REQUIRED LITERALS of its patterns (regex_compile.h): the interval search,
// the driver choice, hit_lines_kernel (or, under fold, the seed kernels) and terms_verify_kernel ran over them unchanged
// and left one candidate per entry that holds every literal of its group.  Here every candidate is decided: the entry is
// walked once, first byte to last, through the group's DFA of the WHOLE-ENTRY language (the leading and the trailing
// [^\n]* are part of the table, so there is no start position to try).  Under fold the table itself folds: the kernel
// has one form.

// One regex batch's tables as the kernel reads them (SearchRequest's regex block, on the device; RegexBlock).
struct RegexTables {
    const u32 *hdr;         // REGEX_HDR_WORDS per group (RegexHdr)
    const u8 *cls;          // 256 per group
    const u16 *tab;         // every group's nstates x ncls, at hdr[RX_TABLE]
};

// One lane per candidate, grid-stride.  The entry is [s, end), end as terms_verify_kernel has it: the closing newline, or n
// for an unterminated last entry.  Eight bytes of text per step in one unaligned load; their eight classes are looked up
// together (they do not depend on the state), then up to eight dependent table loads follow, masked to the bytes inside the
// entry -- a byte behind `end` (the newline, the next entry, the padding) is never taken.  State 0 and the sink absorb, so
// the two are tested once per step.  Keeps the candidate iff the last state accepts; writes len[t] = kSkip of its own
// candidate and nothing else.  No LDS, no scratch, no ballot: the lanes are independent.
// BOUNDS.  t < H indexes len, start and, through pair_of_hit, hit_off; g < ngroups and c < nc follow from a < ngq = ngroups
// x nc.  Text: p < end <= n and the load takes text[p, p + 8), at most 7 bytes past n -- the text is readable 128 bytes past
// n.  cls: an index < 256 into the group's 256 bytes.  Table: regex_request_ok (search_layout.h) has held every group to
// table + nstates x ncls <= the tables' size, start < nstates, every byte of its class map < ncls and every entry of its
// table < nstates, so state x ncls + class stays inside the group's table by induction over the walk.  The loop runs
// (end - s + 7) / 8 trips at most.
__global__ __launch_bounds__(256) void regex_verify_kernel(const ChunkDesc *chunks, u32 nc, RegexTables rx, u64 ngq, const u64 *hit_off,
                                                             u64 H, const u32 *start, u32 *len)
{
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += step) {
        const u32 l = len[t];
        if (l == kSkip) continue;
        const u64 a = pair_of_hit(hit_off, ngq, t);
        const u32 g = (u32)(a / nc), c = (u32)(a % nc);
        const ChunkDesc ch = chunks[c];
        const u32 s = start[t], e = s + l;                       // e <= n - 1: the closing newline, or the last byte
        const u32 end = ch.text[e] == '\n' ? e : ch.n;
        const u32 *h = rx.hdr + (size_t)g * REGEX_HDR_WORDS;
        const u32 ncls = h[RX_NCLS], first_accept = h[RX_FIRST_ACCEPT], sink = h[RX_SINK];
        const u8 *cls = rx.cls + (size_t)g * 256;
        const u16 *tab = rx.tab + h[RX_TABLE];
        u32 state = h[RX_START];
        for (u32 p = s; p < end && state != 0 && state != sink; p += 8) {
            const u64 w = load_u64_unaligned(ch.text + p);
            const u32 m = end - p;                               // bytes of this step inside the entry (8 or more: all)
            u32 k[8];
#pragma unroll
            for (u32 i = 0; i < 8; ++i) k[i] = cls[(u32)(w >> (8 * i)) & 0xffu];
#pragma unroll
            for (u32 i = 0; i < 8; ++i)
                if (i < m) state = tab[state * ncls + k[i]];
        }
        if (state < first_accept) len[t] = kSkip;
    }
}
