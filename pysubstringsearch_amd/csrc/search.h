// search.h -- batched device search entry point (see search.hip).
#pragma once
#include "common.h"
#include "search_layout.h"      // SearchMode, SearchRequest, the rules and the layouts of the batch driver
#include "span_core.h"          // kSpanPatPad: what the host leaves behind the patterns of a span batch

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

// Match spans of `rows` (resident chunk, line) pairs the caller has validated, row i against pattern pat_of[i] of the nq
// patterns (span_impl.h): out receives 3 x int32 per row -- start, length, distance, or -1, 0, -1 -- in the order asked.
// The patterns are folded to lower case already where `fold`, and kSpanPatPad zero bytes follow them; pvoid[q] != 0
// marks a pattern that holds a newline (all its rows are no match).  One wait on the stream.
int match_spans_device(DeviceCtx *ctx, const ChunkDesc *d_chunks, const LineDesc *d_lines, const uint32_t *chunk_of, const uint32_t *line_of,
                       const uint32_t *pat_of, uint64_t rows, const uint8_t *pbytes, const uint64_t *poff, uint32_t nq, const uint8_t *budget,
                       const uint8_t *pvoid, bool edits, bool fold, int32_t *out);

// Merge of `world` packed results of the same nq queries, all resident on ctx's device, into one (query-major,
// rank-major inside a query -- pss_merge_packed's order) on the same device.  starts[r] = entry starts (no closing
// offset); out_offsets receives sum(num_entries) + 1 entries.  Synchronises the stream.
int merge_packed_device(DeviceCtx *ctx, uint32_t world, uint64_t nq, const void *const *d_counts, const void *const *d_starts,
                        const void *const *d_bytes, const uint64_t *num_entries, const uint64_t *num_bytes, void *d_out_counts,
                        void *d_out_offsets, void *d_out_bytes);

}  // namespace pss
