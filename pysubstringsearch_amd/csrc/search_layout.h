// search_layout.h -- what the host driver of a search batch (search.hip, Batch) decides by and carves, stated once: the
// request, the constants its routes read, the rules a request must keep and the routes a batch may take as pure
// functions of their arguments, and ONE description of every slot and staging area the driver carves by hand (offsets
// of the regions and an end, functions of the sizes alone).  Plain C++ without HIP, like rounds_layout.h, msd_layout.h
// and build_plan.h: everything here is arithmetic (tests/native/search_layout.cpp restates it on the CPU).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pss.h"

namespace pss {

// ---- the request ---------------------------------------------------------------------------------------------------

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
    //   near_fold, with near_budget alone, with or without near_edits: the budget is counted under ASCII CASE FOLDING
    //   (DESIGN.md 4.19).  term_bytes holds the patterns folded to lower case; a pattern's queries are, piece by piece, the
    //   spellings of the piece's seed (ascending), each at the seed's position inside the PATTERN.  A query is then no
    //   piece: the device computes the pieces' bounds from a pattern's length and budget.  No exclude flag is set.
    const uint8_t *term_bytes = nullptr; const uint64_t *term_offsets = nullptr; uint32_t nterms = 0;
    const uint64_t *seed_offsets = nullptr; const uint32_t *seed_pos = nullptr; const uint8_t *near_budget = nullptr;
    bool near_edits = false;
    bool near_fold = false;
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
    // regex_hdr .. regex_table_words, together with group_offsets and exclude: the groups are the REQUIRED LITERALS of ngroups
    // regular expressions (regex_compile.h) -- an all-terms batch, plain or seeded under fold, whose exclude flags
    // are all zero -- and every candidate the all-terms verify step leaves is walked through its group's DFA (regex_impl.h):
    //   regex_hdr: REGEX_HDR_WORDS words per group -- the offset of its table inside regex_tables in u16 units, nstates, ncls,
    //     start, first_accept, sink, anchors, 0;
    //   regex_cls: 256 bytes per group, the class of every byte (< ncls);
    //   regex_tables: regex_table_words u16 in all, per group nstates x ncls of them, every one < nstates.
    // The caller has compiled all of it (capi_reader_impl.h, regex_batch).  Not with anchors, seq_anchors, a class block, budgets,
    // SEARCH_DEVICE or low_latency.
    const uint32_t *regex_hdr = nullptr; const uint8_t *regex_cls = nullptr; const uint16_t *regex_tables = nullptr;
    uint64_t regex_table_words = 0;
    // any_term_alts .. any_nalts, together with the seeded block and no budgets: an ANY-OF batch (any_impl.h).  The
    // groups are the ngroups = nterms SETS, one include term each (identity group_offsets, zero exclude flags); term_bytes holds
    // a set's ALTERNATIVES back to back -- normalised (any_terms.h): no 0x0A, none a substring of another, ascending; folded to
    // lower case where the queries are spellings --, and a query belongs to one alternative, no longer to the whole term:
    //   any_term_alts (nterms + 1): the alternatives of set t are any_term_alts[t] .. any_term_alts[t + 1];
    //   any_alt_offsets (any_nalts + 1): alternative j is term_bytes[any_alt_offsets[j], any_alt_offsets[j + 1]), not empty;
    //   any_query_alt (nq): the alternative query v was taken from; seed_pos[v] is its position inside THAT alternative.
    // any_fold: the alternatives are compared under ASCII case folding -- they are folded to lower case, and a query is a
    // spelling of its alternative's seed; else a query is its alternative, at position 0.
    // A set may have no alternative left (all of them held a 0x0A): it has no query and matches nothing.  Not with anchors,
    // seq_anchors, a class block, budgets, a regex block, SEARCH_DEVICE or low_latency.
    const uint64_t *any_term_alts = nullptr, *any_alt_offsets = nullptr; const uint32_t *any_query_alt = nullptr;
    uint32_t any_nalts = 0;
    bool any_fold = false;
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

// ---- the constants the routes read ---------------------------------------------------------------------------------

constexpr uint32_t SM_MAX_VQ = 1024;            // (query, chunk) pairs the fused small-batch path takes
constexpr uint32_t SM_MAX_PLEN = 256;           // longest query that path takes (kept in LDS)
constexpr uint32_t SM_BLOCK_MAX_VQ = 64;        // pairs that get one workgroup each; the resident kernel's limit
constexpr uint32_t MID_MAX = 65536;             // pairs (and hits) of the mid pipeline: one workgroup's scan
constexpr size_t SM_OFF_QUERY = 32768;          // in the pinned scratch: a tiny batch's query bytes, ...
constexpr size_t SM_QUERY_ROOM = 8192;          // ... that many at most with their 32 zero bytes, then as many of offsets
constexpr size_t SEARCH_STAGE_Q = (size_t)2 << 20, SEARCH_STAGE_R = (size_t)4 << 20;      // pinned staging: queries up | results down
constexpr uint32_t SEARCH_SCAN_BLOCKS = 1024;   // SC_MAX_BLOCKS of scan.h (which needs HIP): partial sums of a device_excl_scan
constexpr size_t SEARCH_PAD = 32;               // zero bytes behind every byte array a kernel reads past the end of
constexpr uint32_t REGEX_HDR_WORDS = 8;         // u32 per group of a regex batch: table offset, nstates, ncls, start, first_accept, sink, anchors, 0
enum RegexHdr { RX_TABLE = 0, RX_NSTATES = 1, RX_NCLS = 2, RX_START = 3, RX_FIRST_ACCEPT = 4, RX_SINK = 5, RX_ANCHORS = 6 };
constexpr uint32_t REGEX_STATES_MAX = 4096;     // PSS_REGEX_MAX_STATES
constexpr uint64_t REGEX_TABLE_WORDS_MAX = (uint64_t)32 << 20;      // 64 MiB of u16 in one batch

// ---- the rules a request keeps -------------------------------------------------------------------------------------
// The C ABI validates a batch before it builds a request, so these state what search_batch_device relies on; it turns a
// verdict into its message and PSS_EINVAL.  In the order they are judged:
enum RequestVerdict {
    REQUEST_OK = 0,
    REQUEST_IDS_WITHOUT_LINES,      // the ids mode over chunks without line tables
    REQUEST_ANCHORED,               // anchors with SEARCH_DEVICE or low_latency
    REQUEST_ALL_TERMS,              // groups with anchors, without exclude flags or sequence anchors, with SEARCH_DEVICE or low_latency
    REQUEST_SEEDED,
    REQUEST_CLASS,
    REQUEST_REGEX,
    REQUEST_ANY,
};

// A seeded batch carries its groups, its terms and the queries' offsets and positions, and either exclude flags or sequence
// anchors; it excludes anchors, SEARCH_DEVICE and low_latency; a budget adds: identity groups of one include term each, no
// sequence anchors; near_edits says how a budget is counted and is legal with one alone; near_fold says that it is counted
// under fold, is legal with one alone too, and then no term excludes and there is no class block.
inline bool seeded_request_ok(const SearchRequest &rq)
{
    bool ok = rq.seed_offsets && rq.seed_pos && rq.group_offsets && rq.term_bytes && rq.term_offsets &&
              (!rq.nterms || rq.exclude || rq.seq_anchors) && !rq.anchors && rq.mode != SEARCH_DEVICE && !rq.low_latency;
    ok = ok && (rq.near_budget || !rq.near_edits);
    ok = ok && (!rq.near_fold || (rq.near_budget && !rq.seq_anchors && !rq.class_bytes && rq.exclude));
    for (uint32_t t = 0; ok && rq.near_fold && t < rq.nterms; ++t) ok = rq.exclude[t] == 0;
    if (rq.near_budget) {
        ok = ok && !rq.seq_anchors && rq.exclude && rq.ngroups == rq.nterms;
        for (uint32_t g = 0; ok && g < rq.ngroups; ++g) ok = rq.group_offsets[g] == g && rq.group_offsets[g + 1] == (uint64_t)g + 1;
    }
    return ok;
}

// A class batch is a sequence batch (groups and sequence anchors) that states all of its block, the sets where it names
// any; its terms are cores, so there are at most as many of them as segments; budgets are another search.
inline bool class_request_ok(const SearchRequest &rq)
{
    return rq.class_bytes && rq.class_plane && rq.class_offsets && rq.class_groups && rq.class_cores && rq.class_void &&
           (rq.class_sets || !rq.class_nsets) && rq.class_nsets <= 255 && rq.group_offsets && rq.seq_anchors && !rq.near_budget &&
           (rq.seed_offsets ? rq.nterms : rq.nq) <= rq.class_nsegs && rq.class_groups[0] == 0 &&
           rq.class_groups[rq.ngroups] == rq.class_nsegs;
}

// A regex batch is an all-terms batch (groups and exclude flags, none set) that states its headers, class maps and tables;
// every group's table lies inside the tables, its numbers inside its table, every class of its map below ncls and every entry
// of its table below nstates -- all that regex_verify_kernel's reads rest on (one pass over what goes up anyway).
inline bool regex_request_ok(const SearchRequest &rq)
{
    bool ok = rq.regex_hdr && rq.regex_cls && rq.regex_tables && rq.group_offsets && rq.exclude && !rq.anchors && !rq.seq_anchors &&
              !rq.class_bytes && !rq.near_budget && rq.mode != SEARCH_DEVICE && !rq.low_latency &&
              rq.regex_table_words <= REGEX_TABLE_WORDS_MAX;
    const uint32_t nt = rq.seed_offsets ? rq.nterms : rq.nq;
    for (uint32_t t = 0; ok && t < nt; ++t) ok = rq.exclude[t] == 0;
    for (uint32_t g = 0; ok && g < rq.ngroups; ++g) {
        const uint32_t *h = rq.regex_hdr + (size_t)g * REGEX_HDR_WORDS;
        ok = h[RX_NSTATES] >= 1 && h[RX_NSTATES] <= REGEX_STATES_MAX && h[RX_NCLS] >= 1 && h[RX_NCLS] <= 256 &&
             (uint64_t)h[RX_TABLE] + (uint64_t)h[RX_NSTATES] * h[RX_NCLS] <= rq.regex_table_words && h[RX_START] < h[RX_NSTATES] &&
             h[RX_FIRST_ACCEPT] >= 1 && h[RX_FIRST_ACCEPT] <= h[RX_NSTATES] && h[RX_SINK] < h[RX_NSTATES] && h[RX_ANCHORS] <= 3;
        const uint8_t *cls = rq.regex_cls + (size_t)g * 256;
        for (uint32_t b = 0; ok && b < 256; ++b) ok = cls[b] < h[RX_NCLS];
        const uint16_t *tab = rq.regex_tables + h[RX_TABLE];
        for (size_t i = 0, n = ok ? (size_t)h[RX_NSTATES] * h[RX_NCLS] : 0; ok && i < n; ++i) ok = tab[i] < h[RX_NSTATES];
    }
    return ok;
}

// An any-of batch is a seeded batch of identity groups without an exclude term that states all of its block, and nothing of
// another search.  The offsets are monotone and end where their tables end: the alternatives tile every term, the queries
// are dealt out term by term.  Every query's alternative is one of its term's, and the query fits into it behind its
// position -- all that AnyMatch's reads rest on (any_impl.h): the window it compares is the alternative's, found from the
// query's hit by a position that cannot leave it.
inline bool any_request_ok(const SearchRequest &rq)
{
    bool ok = rq.any_term_alts && rq.any_alt_offsets && rq.any_query_alt && rq.seed_offsets && rq.seed_pos && rq.group_offsets &&
              rq.term_bytes && rq.term_offsets && rq.exclude && (rq.qoffsets || !rq.nq) && !rq.anchors && !rq.seq_anchors &&
              !rq.class_bytes && !rq.near_budget && !rq.near_edits && !rq.near_fold && !rq.regex_hdr && rq.mode != SEARCH_DEVICE &&
              !rq.low_latency && rq.ngroups == rq.nterms;
    if (!ok) return false;
    const uint32_t nt = rq.nterms, na = rq.any_nalts;
    ok = rq.any_term_alts[0] == 0 && rq.any_term_alts[nt] == na && rq.any_alt_offsets[0] == 0 && rq.term_offsets[0] == 0 &&
         rq.any_alt_offsets[na] == rq.term_offsets[nt] && rq.seed_offsets[0] == 0 && rq.seed_offsets[nt] == rq.nq;
    for (uint32_t j = 0; ok && j < na; ++j)
        ok = rq.any_alt_offsets[j] < rq.any_alt_offsets[j + 1] && rq.any_alt_offsets[j + 1] - rq.any_alt_offsets[j] <= 0xffffffffull;
    for (uint32_t t = 0; ok && t < nt; ++t) {
        const uint64_t j0 = rq.any_term_alts[t], j1 = rq.any_term_alts[t + 1], v0 = rq.seed_offsets[t], v1 = rq.seed_offsets[t + 1];
        ok = rq.group_offsets[t] == t && rq.group_offsets[t + 1] == (uint64_t)t + 1 && rq.exclude[t] == 0 && j0 <= j1 && j1 <= na &&
             v0 <= v1 && v1 <= rq.nq && rq.term_offsets[t] <= rq.term_offsets[t + 1] && rq.any_alt_offsets[j0] == rq.term_offsets[t] &&
             rq.any_alt_offsets[j1] == rq.term_offsets[t + 1];
        for (uint64_t v = v0; ok && v < v1; ++v) {
            const uint64_t j = rq.any_query_alt[v];
            ok = j >= j0 && j < j1 && rq.qoffsets[v] <= rq.qoffsets[v + 1] &&
                 (uint64_t)rq.seed_pos[v] + (rq.qoffsets[v + 1] - rq.qoffsets[v]) <= rq.any_alt_offsets[j + 1] - rq.any_alt_offsets[j];
            // (exact bytes: nothing is compared behind the lookup, so the query IS the alternative)
            ok = ok && (rq.any_fold || (rq.seed_pos[v] == 0 && rq.qoffsets[v + 1] - rq.qoffsets[v] == rq.any_alt_offsets[j + 1] - rq.any_alt_offsets[j]));
        }
    }
    return ok;
}

// nc: resident chunks; have_lines: their line tables were built.
inline RequestVerdict check_request(const SearchRequest &rq, uint32_t nc, bool have_lines)
{
    if (rq.mode == SEARCH_IDS && nc && !have_lines) return REQUEST_IDS_WITHOUT_LINES;
    if (rq.anchors && (rq.mode == SEARCH_DEVICE || rq.low_latency)) return REQUEST_ANCHORED;
    if (rq.group_offsets && (rq.anchors || (rq.nq && !rq.exclude && !rq.seq_anchors) || rq.mode == SEARCH_DEVICE || rq.low_latency))
        return REQUEST_ALL_TERMS;
    if ((rq.seed_offsets || rq.seed_pos || rq.near_budget || rq.near_edits || rq.near_fold) && !seeded_request_ok(rq)) return REQUEST_SEEDED;
    if ((rq.class_bytes || rq.class_plane || rq.class_offsets || rq.class_groups || rq.class_cores || rq.class_sets || rq.class_void ||
         rq.class_nsegs || rq.class_nsets) &&
        !class_request_ok(rq))
        return REQUEST_CLASS;
    if ((rq.regex_hdr || rq.regex_cls || rq.regex_tables || rq.regex_table_words) && !regex_request_ok(rq)) return REQUEST_REGEX;
    if ((rq.any_term_alts || rq.any_alt_offsets || rq.any_query_alt || rq.any_nalts || rq.any_fold) && !any_request_ok(rq)) return REQUEST_ANY;
    return REQUEST_OK;
}

// ---- the batch's shape ---------------------------------------------------------------------------------------------
// A valid request normalised once: nothing in the driver asks for a mode again.  nc: resident chunks (> 0); qtotal: bytes
// of the queries as they are searched (an anchored batch: rewritten, anchored_impl.h); the three switches of SearchKnobs.
struct BatchShape {
    bool counts, device, ids, anchored, terms;
    bool seq;                           // terms, and the groups are ordered sequences (sequence_impl.h)
    bool seqc;                          // seq, and the segments hold byte classes: the terms are their cores (seq_class_impl.h)
    bool seeded;                        // terms looked up through seed queries: group -> terms -> queries (seed_impl.h)
    bool near;                          // ... within k mismatches (near_impl.h); else under fold (fold_impl.h, 4.14)
    bool edits;                         // near, and the budget counts edits: EditMatch in NearMatch's place (edit_impl.h, 4.17)
    bool fold_near;                     // near, and the budget is counted under fold: the <true> forms of either Match (4.19)
    bool regex;                         // terms, and every candidate is walked through its group's DFA (regex_impl.h, 4.21)
    bool any;                           // seeded, and a term is a set of alternatives: AnyMatch, exact or under fold (any_impl.h, 4.22)
    bool any_fold;                      // any, under fold: the queries are spellings of the alternatives' seeds
    bool sa_order;
    // An all-terms batch (all_terms_impl.h) has a second pair space: its nq queries are terms, its result rows are the ng
    // groups, and everything from the first scan on runs over (group, chunk) pairs.  For every other batch the two agree.
    uint32_t nrow;                      // rows of the result: groups of an all-terms batch, else queries
    uint64_t nvq;                       // (query, chunk) pairs: what the interval search runs over
    uint64_t nrp;                       // (row, chunk) pairs: what the scans, the hit kernels and the emit kernels run over
    uint32_t nterm;                     // terms of a seeded batch (else 0) ...
    uint64_t ntp;                       // ... and its (term, chunk) pairs
    size_t off_bytes;                   // the queries' offsets
    bool tiny;                          // queries and offsets fit the 16 KiB of the pinned scratch
    bool fused_ok, resident_ok, mid_ok; // routes this batch may take (each may still overflow into the next)

    BatchShape(const SearchRequest &rq, uint32_t nc, uint64_t qtotal, bool no_small_path, bool no_block_path, bool no_mid_pipeline)
    {
        counts = rq.mode == SEARCH_COUNTS;
        device = rq.mode == SEARCH_DEVICE;
        ids = rq.mode == SEARCH_IDS;
        anchored = rq.anchors != nullptr;
        terms = rq.group_offsets != nullptr;
        seq = terms && rq.seq_anchors != nullptr;
        seqc = seq && rq.class_bytes != nullptr;
        seeded = terms && rq.seed_offsets != nullptr;
        near = seeded && rq.near_budget != nullptr;
        edits = near && rq.near_edits;
        fold_near = near && rq.near_fold;
        regex = terms && rq.regex_hdr != nullptr;
        any = seeded && rq.any_term_alts != nullptr;
        any_fold = any && rq.any_fold;
        // (counts do not depend on the order; one hit per entry has one order; an all-terms batch keeps its driver's text order)
        sa_order = rq.sa_order && !counts && !anchored && !terms;
        nrow = rq.rows();
        nvq = (uint64_t)rq.nq * nc;
        nrp = (uint64_t)nrow * nc;
        nterm = rq.seed_offsets ? rq.nterms : 0u;
        ntp = (uint64_t)nterm * nc;
        off_bytes = ((size_t)rq.nq + 1) * 8;
        tiny = !anchored && qtotal + SEARCH_PAD <= SM_QUERY_ROOM && off_bytes <= SM_QUERY_ROOM;
        const bool plain = !anchored && !terms && !sa_order;    // entries that contain the pattern, in text order
        fused_ok = plain && rq.mode == SEARCH_FULL && tiny && nvq <= SM_MAX_VQ && !no_small_path;
        for (uint32_t i = 0; fused_ok && i < rq.nq; ++i) fused_ok = rq.qoffsets[i + 1] - rq.qoffsets[i] <= SM_MAX_PLEN;
        resident_ok = fused_ok && rq.low_latency && rq.nq == 1 && nvq <= SM_BLOCK_MAX_VQ && !no_block_path;
        mid_ok = plain && (rq.mode == SEARCH_FULL || device) && nvq <= MID_MAX && !no_mid_pipeline;
    }
};

// ---- the layouts ---------------------------------------------------------------------------------------------------
// Members are byte offsets from the layout's base; `end` is the offset behind the last region: what the driver reserves.

namespace search_detail {
inline size_t up64(size_t x) { return (x + 63) / 64 * 64; }
// Regions one behind the other, every start on a multiple of 64 bytes.
struct Carver {
    size_t o = 0;
    size_t operator()(size_t bytes)
    {
        const size_t at = o;
        o = up64(o + bytes);
        return at;
    }
};
}  // namespace search_detail

// What a sequence batch keeps behind its term flags in Q_TERMS: one anchor byte per group and, for a class batch, the
// segments as seqc_verify_kernel reads them (SeqClass) -- offsets, the groups' offsets, the cores, the sets, then bytes and
// plane, each with SEARCH_PAD zero bytes behind it (entry_scan reads a core up to 16 bytes past its end).  Offsets from
// the anchor bytes; nothing at all (end = 0) where the batch is no sequence.  Both Q_TERMS layouts embed it.
struct ClassBlock {
    size_t anchors = 0, seg_off = 0, seg_goff = 0, cores = 0, sets = 0, bytes = 0, plane = 0, end = 0;
    ClassBlock() = default;
    // nsegs segments of seg_total positions, nsets sets (read with seqc alone)
    ClassBlock(bool seq, bool seqc, uint32_t nrow, uint32_t nsegs, uint64_t seg_total, uint32_t nsets)
    {
        if (!seq) return;
        search_detail::Carver carve;
        anchors = carve(nrow);
        if (seqc) {
            seg_off = carve(((size_t)nsegs + 1) * 8);
            seg_goff = carve(((size_t)nrow + 1) * 8);
            cores = carve((size_t)nsegs * 8);
            sets = carve((size_t)nsets * 32);
            bytes = carve((size_t)seg_total + SEARCH_PAD);
            plane = carve((size_t)seg_total + SEARCH_PAD);
        }
        end = carve.o;
    }
};

// What a regex batch keeps behind the sequence's block in Q_TERMS, as regex_verify_kernel reads it (RegexTables): the
// headers, the class maps, the tables.  Offsets from its own start; nothing at all (end = 0) where the batch is no regex
// batch.  Both Q_TERMS layouts embed it.
struct RegexBlock {
    size_t hdr = 0, cls = 0, tables = 0, end = 0;
    RegexBlock() = default;
    RegexBlock(bool regex, uint32_t nrow, uint64_t table_words)
    {
        if (!regex) return;
        search_detail::Carver carve;
        hdr = carve((size_t)nrow * REGEX_HDR_WORDS * 4);
        cls = carve((size_t)nrow * 256);
        tables = carve((size_t)table_words * 2);
        end = carve.o;
    }
};

// What an any-of batch keeps behind everything else in Q_TERMS, as AnyMatch reads it (AnyAlts of seed_impl.h): the three
// pointers themselves, the alternatives of every term, the alternatives' offsets into the terms' bytes, every query's
// alternative.  Offsets from its own start; nothing at all (end = 0) where the batch is no any-of batch.
struct AnyBlock {
    size_t hdr = 0, talts = 0, aoff = 0, qalt = 0, end = 0;
    AnyBlock() = default;
    AnyBlock(bool any, uint32_t nterm, uint32_t nalts, uint32_t nq)
    {
        if (!any) return;
        search_detail::Carver carve;
        hdr = carve(3 * sizeof(void *));
        talts = carve(((size_t)nterm + 1) * 8);
        aoff = carve(((size_t)nalts + 1) * 8);
        qalt = carve((size_t)nq * 4);
        end = carve.o;
    }
};

// Slot Q_TERMS of an all-terms or a sequence batch of nq terms in nrow groups: group offsets, term flags, the sequence's
// block, a regex batch's block, then per (group, chunk) pair the driver term, its interval and its hits -- three arrays
// back to back.
struct TermsLayout {
    ClassBlock cls;             // at `anchors`
    RegexBlock rx;              // at `regex`
    size_t goff, tflags, anchors, regex, gdrv, lo, cnt, end;
    TermsLayout(uint32_t nrow, uint32_t nq, uint64_t nrp, const ClassBlock &block, const RegexBlock &rblock = RegexBlock())
        : cls(block), rx(rblock)
    {
        search_detail::Carver carve;
        goff = carve(((size_t)nrow + 1) * 8);
        tflags = carve(nq);
        anchors = carve(cls.end);
        regex = carve(rx.end);
        gdrv = carve.o;
        lo = gdrv + (size_t)nrp * 4;
        cnt = lo + (size_t)nrp * 4;
        end = cnt + (size_t)nrp * 4;
    }
};

// Slot Q_TERMS of a seeded batch: nq seed queries of nterm terms (term_total bytes) in nrow groups.  The queries' offsets
// per term, the terms' offsets, a near batch's overflow word, every query's position inside its term, void flags and term
// flags per term, a near batch's budgets, the sequence's block, a regex batch's block, the terms' bytes (SEARCH_PAD zero
// bytes behind them), the seed hits per (term, chunk) pair, then per (group, chunk) pair the driver term and its hits, back
// to back, then an any-of batch's block.  `over` and `budget` have room in a near batch alone (elsewhere they coincide
// with their neighbours and are not used); an any-of batch is carved as a near batch for the sake of `over` and leaves
// `budget` unused.  `any` is the next multiple of 64 behind the hits where there is a block, else `end` is where it always was.
struct SeedLayout {
    ClassBlock cls;             // at `anchors`
    RegexBlock rx;              // at `regex`
    AnyBlock alts;              // at `any`
    size_t goff, soff, foff, over, pos, fvoid, tflags, budget, anchors, regex, fbytes, tcnt, gdrv, cnt, any, end;
    SeedLayout(uint32_t nrow, uint32_t nterm, uint32_t nq, uint64_t term_total, uint64_t ntp, uint64_t nrp, bool near,
               const ClassBlock &block, const RegexBlock &rblock = RegexBlock(), const AnyBlock &ablock = AnyBlock())
        : cls(block), rx(rblock), alts(ablock)
    {
        search_detail::Carver carve;
        goff = carve(((size_t)nrow + 1) * 8);
        soff = carve(((size_t)nterm + 1) * 8);
        foff = carve(((size_t)nterm + 1) * 8);
        over = carve(near ? 64 : 0);
        pos = carve((size_t)nq * 4);
        fvoid = carve(nterm);
        tflags = carve(nterm);
        budget = carve(near ? nterm : 0);
        anchors = carve(cls.end);
        regex = carve(rx.end);
        fbytes = carve((size_t)term_total + SEARCH_PAD);
        tcnt = carve((size_t)ntp * 4);
        gdrv = carve.o;
        cnt = gdrv + (size_t)nrp * 4;
        any = end = cnt + (size_t)nrp * 4;
        if (alts.end) {
            any = search_detail::up64(end);
            end = any + alts.end;
        }
    }
};

// Slot Q_ANCHOR of an anchored batch: one flag byte per query, then the chunk-edge hits per (query, chunk) pair.
struct AnchorFlags {
    size_t flags, edge, end;
    AnchorFlags(uint32_t nq, uint64_t nvq)
    {
        search_detail::Carver carve;
        flags = carve(nq);
        edge = carve.o;
        end = edge + (size_t)nvq;
    }
};

// Slot Q_SMALL, in 8-byte WORDS: the partial sums of a device_excl_scan, its total behind them, and from 8 words behind
// the total the mid pipeline's MidState.
struct SmallWords {
    static constexpr size_t PARTIAL = 0, TOTAL = SEARCH_SCAN_BLOCKS, MID_STATE = TOTAL + 8;
    static constexpr size_t BYTES = SEARCH_SCAN_BLOCKS * 8 + 256;
};

// The 8-byte words at the start of the pinned scratch that the general pipeline reads its totals from: the hits and, once
// they are read, the kept hits (entries); the bytes; a near batch's overflow flag (seed_union_kernel's, fetched by
// seed_drivers and judged with the hit total).  (The mid pipeline's MidState comes down over the same words.)
enum PinnedWord { PW_COUNT = 0, PW_BYTES = 1, PW_NEAR_OVERFLOW = 2 };

// The host copy of queries, offsets and, for an anchored batch, its flag bytes, in one of three places: a tiny batch's in
// the pinned scratch (TINY_*, from the scratch's start); one that fits() in the pinned staging (q, off, flags from the
// staging's start); an anchored batch too large for that in two vectors of its own (own_bytes of queries and, at
// own_flags, flags; the offsets apart).  A plain batch too large for the staging goes up from the caller's memory.
struct QueryStage {
    static constexpr size_t TINY_Q = SM_OFF_QUERY, TINY_OFF = SM_OFF_QUERY + SM_QUERY_ROOM;
    size_t q = 0, off, flags, staged, own_flags, own_bytes;
    QueryStage(bool anchored, uint32_t nq, uint64_t qtotal, size_t off_bytes)
    {
        const size_t q_room = search_detail::up64((size_t)qtotal + SEARCH_PAD), o_room = search_detail::up64(off_bytes);
        off = q_room;
        flags = q_room + o_room;
        staged = anchored ? q_room + o_room + nq : (size_t)qtotal + SEARCH_PAD + off_bytes + 64;
        own_flags = q_room;
        own_bytes = q_room + nq;
    }
    bool fits() const { return staged <= SEARCH_STAGE_Q; }
};

// The result of download_result on its way through the pinned staging, from SEARCH_STAGE_Q behind the staging's start:
// E entry starts, B bytes, nrow counts.
struct ResultStage {
    size_t offsets, bytes, counts, end;
    ResultStage(uint64_t E, uint64_t B, uint32_t nrow)
    {
        search_detail::Carver carve;
        offsets = carve((size_t)E * 8);
        bytes = carve((size_t)B);
        counts = carve.o;
        end = counts + (size_t)nrow * 8;
    }
    bool fits() const { return end <= SEARCH_STAGE_R; }
};

}  // namespace pss
