// search.h -- batched device search entry point (see search.hip).
#pragma once
#include "common.h"

namespace pss {

// One resident chunk: text (n bytes, zero padded and readable 128 bytes past the end), its
// suffix array (n x u32) and a table of key samples: skeys[j] = the first 8 bytes of suffix
// sa[j << shift] as a big-endian integer (ceil(n / 2^shift) entries, nullptr = none).  The
// keys are non-decreasing along the suffix array, so two searches in the small table (L2
// resident) confine a query to a window of one or two strides before the suffix array and
// the text are touched.
struct ChunkDesc {
    const uint8_t *text;
    const uint32_t *sa;
    const uint64_t *skeys;
    uint32_t n;
    uint32_t shift;
};
constexpr uint32_t kSampleShift = 11;   // one key sample per 2048 suffixes: 2 MiB per 512 MiB chunk

// Entries of the key-sample table of an n-byte chunk, and the kernel launch that fills it
// (stream-ordered on ctx->stream; `skeys` must hold sample_count(n, shift) entries).
static inline uint64_t sample_count(uint32_t n, uint32_t shift) { return ((uint64_t)n + (1u << shift) - 1) >> shift; }
int build_key_samples(DeviceCtx *ctx, const uint8_t *d_text, const uint32_t *d_sa, uint32_t n, uint32_t shift,
                      uint64_t *d_skeys);

// Line index of one resident chunk (line_index_impl.h): what turns the start of an entry into its number inside the chunk
// and back.  rank[j] = newlines in text[0, j << shift), j = 0 .. nblocks; rank[nblocks + 1] = entries.  Kept beside
// ChunkDesc, in a parallel array indexed by chunk, because every search kernel copies ChunkDesc by value and only the
// two id kernels need this.  file_index = the chunk's index in the index file: the high word of its entry ids.
struct LineDesc {
    const uint32_t *rank;
    uint32_t nblocks;
    uint32_t shift;
    uint32_t entries;
    uint32_t file_index;
};
constexpr uint32_t kLineShift = 8;      // blocks of 256 bytes: the table is 1/64 of the text ("Entry ids")
constexpr uint32_t kLineShiftMin = 6, kLineShiftMax = 10;     // one group of 4 .. 64 lanes counts a block
static inline uint64_t line_blocks(uint32_t n, uint32_t shift) { return ((uint64_t)n + (1u << shift) - 1) >> shift; }
static inline size_t line_table_bytes(uint32_t n, uint32_t shift) { return (size_t)(line_blocks(n, shift) + 2) * 4; }
// Fills d_rank (line_table_bytes) for the n-byte text (stream-ordered on ctx->stream).
int build_line_index(DeviceCtx *ctx, const uint8_t *d_text, uint32_t n, uint32_t shift, uint32_t *d_rank);

// Host-side packed result of one batch (owned by pss_result).  Small results are malloc'ed; large
// ones (offsets + bytes) share ONE pinned block from the pool in common.h, so the D2H copy runs at
// link speed.  In SEARCH_DEVICE mode nothing but the totals comes down: d_* point into the device
// context's workspace and stay valid until the next search on that device.
struct HostResult {
    uint64_t nq = 0;
    uint64_t n_entries = 0;
    uint64_t n_bytes = 0;
    uint64_t *qcount = nullptr;    // [nq]
    uint64_t *offsets = nullptr;   // [n_entries + 1]
    uint8_t *bytes = nullptr;
    void *pinned = nullptr;        // when set: offsets and bytes live inside this block
    size_t pinned_bytes = 0;
    const uint64_t *d_qcount = nullptr;    // SEARCH_DEVICE: [nq]
    const uint64_t *d_offsets = nullptr;   //                [n_entries] entry starts
    const uint8_t *d_bytes = nullptr;      //                [n_bytes]
    void release();
};

// Room for E + 1 offsets and B bytes in `res`: one block of the pinned pool when the result is large (the D2H copy then
// runs at link speed), else malloc.
int alloc_host_result(HostResult *res, uint64_t E, uint64_t B, bool allow_pinned);

enum SearchMode {
    SEARCH_FULL = 0,     // packed result on the host
    SEARCH_COUNTS = 1,   // res->qcount only (entries each query would return); no entry is materialised
    SEARCH_DEVICE = 2,   // packed result left on the device (multi-GPU gather over RCCL takes it from there)
    SEARCH_IDS = 3,      // packed result on the host whose "bytes" are one u64 entry id per entry (offsets[i] = 8 i): the general
                         // pipeline up to the kept-hit scan, then one id per kept hit -- no byte scan, no text copy.  Needs d_lines.
};

// One batch as its caller states it.  search_batch_device normalises it once into the few booleans its stages read.
struct SearchRequest {
    const uint8_t *qbytes = nullptr; const uint64_t *qoffsets = nullptr; uint32_t nq = 0;   // nq patterns back to back, nq + 1 offsets
    SearchMode mode = SEARCH_FULL;
    // anchors (nq values, PSS_ANCHOR_START | PSS_ANCHOR_END, validated by the caller): the anchored search of anchored_impl.h --
    // entries that start with, end with or equal the pattern instead of entries that contain it.  Modes FULL, COUNTS and IDS;
    // always the general pipeline, one hit per entry, so sa_order has nothing to order.
    const uint8_t *anchors = nullptr;
    // group_offsets (ngroups + 1 entries into the nq patterns, which are then TERMS) and exclude (nq flags, 0 or 1, validated by
    // the caller like the offsets): the all-terms search of all_terms_impl.h -- per group the entries that contain every include
    // term and no exclude term.  The result's rows are the groups.  Modes FULL, COUNTS and IDS; not with anchors; always the
    // general pipeline, in the plain search's order for each pair's driver term, so sa_order has no say.
    const uint64_t *group_offsets = nullptr; uint32_t ngroups = 0; const uint8_t *exclude = nullptr;
    // seq_anchors (ngroups values, PSS_ANCHOR_START | PSS_ANCHOR_END or 0, validated by the caller), together with group_offsets:
    // the groups are ORDERED SEQUENCES of segments -- the wildcard search of sequence_impl.h: per group the entries that hold
    // its segments left to right without overlap, the first at the entry's start and / or the last at its end when anchored.
    // exclude is then unused and may be null.  Everything else as for an all-terms batch.
    const uint8_t *seq_anchors = nullptr;
    // seed_offsets (nterms + 1 entries into the nq patterns), seed_pos (nq values), term_bytes and term_offsets (nterms + 1),
    // together with group_offsets: a SEEDED batch (seed_impl.h).  The rows are the ngroups groups, group_offsets
    // index the nterms TERMS -- whole patterns, term_bytes back to back, as they are verified --, exclude has nterms flags, and
    // the nq patterns are the terms' exact SEED QUERIES: term t's are seed_offsets[t] .. seed_offsets[t + 1], query v at
    // seed_pos[v] inside its term.  Modes FULL, COUNTS and IDS; not with anchors or low_latency; always the general pipeline,
    // and sa_order has no say.
    //   near_budget null: the case-insensitive search of fold_impl.h -- an all-terms batch (exclude) or a
    //   sequence batch (seq_anchors) under fold; a plain pattern is a group of one include term.  term_bytes holds the terms
    //   folded to lower case, and a term's queries are the spellings of its seed, in ascending byte order, all at the seed's
    //   offset.
    //   near_budget (nterms bytes, 0 .. 3): the search within k mismatches of near_impl.h.  The groups are
    //   the ngroups = nterms patterns, one include term each (identity group_offsets, zero exclude flags, no seq_anchors);
    //   term_bytes holds the patterns themselves -- exact bytes, nothing is folded --, near_budget[t] is pattern t's budget k,
    //   and its queries are its k + 1 pieces, left to right.
    //   near_edits, with near_budget alone: the budget counts EDITS -- insertions, deletions and substitutions of single
    //   bytes (edit_impl.h) -- instead of substitutions.  Everything else of the request is near's.
    const uint8_t *term_bytes = nullptr; const uint64_t *term_offsets = nullptr; uint32_t nterms = 0;
    const uint64_t *seed_offsets = nullptr; const uint32_t *seed_pos = nullptr; const uint8_t *near_budget = nullptr;
    bool near_edits = false;
    // class_bytes .. class_void, together with group_offsets and seq_anchors: a sequence batch whose segments hold BYTE CLASSES
    // (`?`, `[...]`) beside literal bytes (seq_class_impl.h).  The nq patterns -- under fold the nterms terms -- are
    // then the CORES of the segments that have one (a segment's longest run of literal positions), group_offsets index them, and
    // everything up to the verify step runs over cores as over segments.  The block states the segments themselves, which the
    // verify step alone reads:
    //   class_offsets (class_nsegs + 1) cut class_bytes and class_plane into segments, one byte per position: class_plane is 0 at
    //     a literal position, whose byte class_bytes holds (folded to lower case under fold), else the 1-based index of the
    //     position's set, and class_bytes 0;
    //   class_groups (ngroups + 1) cut the segments into the groups, in order;
    //   class_cores holds two values per segment: the core's offset inside the segment and its length -- or, length 0, a segment
    //     without a core, and then 1 in the offset's place iff every position accepts every byte (a run of `?`);
    //   class_sets: class_nsets x 32 bytes, bit b of a set = byte b >> 3, bit b & 7; no set holds 0x0A, none is empty, and under
    //     fold every set is closed under it;
    //   class_void (one flag per core): the core's group holds a literal 0x0A somewhere and matches nothing.
    // The caller has validated all of it (capi_reader_impl.h, seqc_batch).  Not with near_budget.
    const uint8_t *class_bytes = nullptr, *class_plane = nullptr; const uint64_t *class_offsets = nullptr; uint32_t class_nsegs = 0;
    const uint64_t *class_groups = nullptr; const uint32_t *class_cores = nullptr;
    const uint8_t *class_sets = nullptr; uint32_t class_nsets = 0; const uint8_t *class_void = nullptr;
    uint32_t rows() const { return group_offsets ? ngroups : nq; }     // rows of the result: queries, or groups of terms
    bool low_latency = false;            // one query through the resident kernel when it fits (an unanchored SEARCH_FULL batch only)
    // sa_order: the entries of one (query, chunk) pair come out in the reference's order -- suffix-array order of the FIRST hit
    // inside each entry (src/lib.rs:262-276: the hits are walked in suffix-array order and an entry is pushed when its line
    // start is first seen) -- instead of the order of each entry's leftmost match.  Opt-in (pss_reader_set_result_order): it
    // takes the general pipeline and one extra sort of the hits.
    bool sa_order = false;
    // chunk_hits (optional, nc entries): how much of the batch's work landed on every chunk -- suffix-array hits per chunk on
    // the multi-kernel paths, entries per chunk on the fused small-batch path.  The reader's residency manager feeds on it
    // (capi.cpp); it costs one small kernel and a stream synchronisation, so readers whose chunks all live in HBM pass nullptr.
    uint64_t *chunk_hits = nullptr;
};

// Host side of the case-insensitive search (fold_impl.h).  fold_seed: the seed of pat[0, len) -- its longest window with at
// most `letters` ASCII letters, the leftmost on a tie -- into seed_off / seed_len; returns the seed's letter count f.
// fold_spellings: the 2^f spellings of a seed of f letters back to back into out (len << f bytes), ascending bytewise.
uint32_t fold_seed(const uint8_t *pat, uint64_t len, uint32_t letters, uint64_t *seed_off, uint64_t *seed_len);
void fold_spellings(const uint8_t *seed, uint64_t len, uint32_t f, uint8_t *out);

// Host side of the search within k mismatches (near_impl.h): the k + 1 pieces of a pattern of len > k bytes, piece j =
// [off[j], off[j + 1]) with off[j] = j * len / (k + 1); off has k + 2 entries.
void near_pieces(uint64_t len, uint32_t k, uint64_t *off);

// The batch over the nc resident chunks of d_chunks (d_lines: their line tables, parallel to d_chunks; read by SEARCH_IDS
// alone, nullptr where none were built).
int search_batch_device(DeviceCtx *ctx, const ChunkDesc *d_chunks, const LineDesc *d_lines, uint32_t nc, const SearchRequest &rq,
                        HostResult *res, pss_search_stats *st);

// Text of n entries named by (resident chunk, line) pairs the caller has validated (line < entries of that chunk): a
// packed result of n "queries" with one entry each, in the order asked.
int entries_by_id_device(DeviceCtx *ctx, const ChunkDesc *d_chunks, const LineDesc *d_lines, const uint32_t *chunk_of,
                         const uint32_t *line_of, uint64_t n, HostResult *res);

// Merge of `world` packed results of the same nq queries, all resident on ctx's device, into one (query-major,
// rank-major inside a query -- pss_merge_packed's order) on the same device.  starts[r] = entry starts (no closing
// offset); out_offsets receives sum(num_entries) + 1 entries.  Synchronises the stream.
int merge_packed_device(DeviceCtx *ctx, uint32_t world, uint64_t nq, const void *const *d_counts, const void *const *d_starts,
                        const void *const *d_bytes, const uint64_t *num_entries, const uint64_t *num_bytes, void *d_out_counts,
                        void *d_out_offsets, void *d_out_bytes);

}  // namespace pss
