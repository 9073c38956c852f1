// any_request.cpp -- the request rule of an any-of batch (csrc/search_layout.h, any_request_ok) on the CPU:
// one valid request in exact bytes and one under fold, every clause of the rule broken in turn, what BatchShape makes of the
// block, the block's layout against a table restated here, and the normalisation of csrc/any_terms.h on a few sets.  Headers
// only: no library, no device.  (tests/test_any_host.py builds it with g++ under AddressSanitizer + UBSan.)
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "any_terms.h"
#include "search_layout.h"

using namespace pss;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            ++failures;                                      \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

// Three sets: {`ab`, `cde`}, {} (all of its alternatives held a newline), {`f1`}.
// Exact: the queries are the alternatives.  Under fold with one letter: `ab` -> seed `a` at 0 (A a), `cde` -> `c` at 0 (C c),
// `f1` -> `f1` at 0 (F1 f1).
static const uint8_t TERMS[] = "abcdef1";
static const uint64_t TOFF[] = {0, 5, 5, 7};
static const uint64_t TALTS[] = {0, 2, 2, 3};
static const uint64_t AOFF[] = {0, 2, 5, 7};
static const uint64_t IDENT[] = {0, 1, 2, 3};
static const uint8_t NO_EXCLUDE[] = {0, 0, 0}, Z8[8] = {0};
// exact
static const uint64_t X_QOFF[] = {0, 2, 5, 7};
static const uint64_t X_SOFF[] = {0, 2, 2, 3};
static const uint32_t X_POS[] = {0, 0, 0}, X_QALT[] = {0, 1, 2};
// fold
static const uint8_t F_QUERIES[] = "AaCcF1f1";
static const uint64_t F_QOFF[] = {0, 1, 2, 3, 4, 6, 8};
static const uint64_t F_SOFF[] = {0, 4, 4, 6};
static const uint32_t F_POS[] = {0, 0, 0, 0, 0, 0}, F_QALT[] = {0, 0, 1, 1, 2, 2};

static SearchRequest common_rq()
{
    SearchRequest rq;
    rq.mode = SEARCH_IDS;
    rq.group_offsets = IDENT;
    rq.ngroups = 3;
    rq.exclude = NO_EXCLUDE;
    rq.term_bytes = TERMS;
    rq.term_offsets = TOFF;
    rq.nterms = 3;
    rq.any_term_alts = TALTS;
    rq.any_alt_offsets = AOFF;
    rq.any_nalts = 3;
    return rq;
}

static SearchRequest exact_rq()
{
    SearchRequest rq = common_rq();
    rq.qbytes = TERMS;
    rq.qoffsets = X_QOFF;
    rq.nq = 3;
    rq.seed_offsets = X_SOFF;
    rq.seed_pos = X_POS;
    rq.any_query_alt = X_QALT;
    return rq;
}

static SearchRequest fold_rq()
{
    SearchRequest rq = common_rq();
    rq.qbytes = F_QUERIES;
    rq.qoffsets = F_QOFF;
    rq.nq = 6;
    rq.seed_offsets = F_SOFF;
    rq.seed_pos = F_POS;
    rq.any_query_alt = F_QALT;
    rq.any_fold = true;
    return rq;
}

// A copy of an array of the request with one value changed; lives as long as the program (the request points into it).
template <typename T>
static const T *with(const T *src, size_t n, size_t at, T value)
{
    static std::vector<std::vector<T>> keep;
    keep.emplace_back(src, src + n);
    keep.back()[at] = value;
    return keep.back().data();
}

static void broken(const char *what, SearchRequest rq, RequestVerdict want = REQUEST_ANY)
{
    const RequestVerdict got = check_request(rq, 2, true);
    CHECK(got == want, "%s: verdict %d, want %d", what, (int)got, (int)want);
}

static void rules()
{
    CHECK(check_request(exact_rq(), 2, true) == REQUEST_OK, "the exact request");
    CHECK(check_request(fold_rq(), 2, true) == REQUEST_OK, "the fold request");
    for (SearchMode mode : {SEARCH_FULL, SEARCH_COUNTS, SEARCH_IDS}) {
        SearchRequest rq = fold_rq();
        rq.mode = mode;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "mode %d", (int)mode);
    }
    for (bool fold : {false, true}) {
        const auto base = [&] { return fold ? fold_rq() : exact_rq(); };
        const uint32_t nq = base().nq;
        SearchRequest rq;
        // the block states all of itself
        rq = base(); rq.any_term_alts = nullptr; broken("no alternatives per term", rq);
        rq = base(); rq.any_alt_offsets = nullptr; broken("no alternative offsets", rq);
        rq = base(); rq.any_query_alt = nullptr; broken("no alternative per query", rq);
        rq = base(); rq.seed_offsets = nullptr; rq.seed_pos = nullptr; broken("no seeded block", rq);
        rq = base(); rq.exclude = nullptr; broken("no exclude flags", rq, REQUEST_ALL_TERMS);
        // nothing of another search
        rq = base(); rq.near_budget = Z8; broken("with budgets", rq);
        rq = base(); rq.near_budget = Z8; rq.near_edits = true; broken("with budgets that count edits", rq);
        rq = base(); rq.near_budget = Z8; rq.near_fold = true; broken("with budgets under fold", rq);
        rq = base(); rq.seq_anchors = Z8; broken("with sequence anchors", rq);
        rq = base(); rq.exclude = with(NO_EXCLUDE, 3, 2, (uint8_t)1); broken("with a term that excludes", rq);
        rq = base(); rq.anchors = Z8; broken("with anchors", rq, REQUEST_ALL_TERMS);
        rq = base(); rq.mode = SEARCH_DEVICE; broken("to a device result", rq, REQUEST_ALL_TERMS);
        rq = base(); rq.low_latency = true; broken("low latency", rq, REQUEST_ALL_TERMS);
        {
            static const uint32_t HDR[3 * REGEX_HDR_WORDS] = {0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0};
            static const uint8_t CLS[3 * 256] = {0};
            static const uint16_t TAB[1] = {0};
            rq = base(); rq.regex_hdr = HDR; rq.regex_cls = CLS; rq.regex_tables = TAB; rq.regex_table_words = 1;
            broken("with a regex block", rq);
        }
        // identity groups of one term each
        rq = base(); rq.ngroups = 2; broken("fewer groups than terms", rq);
        rq = base(); rq.group_offsets = with(IDENT, 4, 1, (uint64_t)2); broken("a group of two terms", rq);
        // every offset monotone and inside its table
        rq = base(); rq.any_term_alts = with(TALTS, 4, 0, (uint64_t)1); broken("the terms' alternatives start at 1", rq);
        rq = base(); rq.any_term_alts = with(TALTS, 4, 3, (uint64_t)2); broken("the terms' alternatives end before the last", rq);
        rq = base(); rq.any_term_alts = with(TALTS, 4, 3, (uint64_t)4); broken("the terms' alternatives end behind the last", rq);
        rq = base(); rq.any_term_alts = with(TALTS, 4, 1, (uint64_t)3); broken("the terms' alternatives decrease", rq);
        rq = base(); rq.any_nalts = 4; broken("more alternatives than offsets", rq);
        rq = base(); rq.any_alt_offsets = with(AOFF, 4, 0, (uint64_t)1); broken("the alternatives start at 1", rq);
        rq = base(); rq.any_alt_offsets = with(AOFF, 4, 1, (uint64_t)0); broken("an empty alternative", rq);
        rq = base(); rq.any_alt_offsets = with(AOFF, 4, 1, (uint64_t)6); broken("the alternatives decrease", rq);
        rq = base(); rq.any_alt_offsets = with(AOFF, 4, 3, (uint64_t)8); broken("the alternatives end behind the terms", rq);
        rq = base(); rq.any_alt_offsets = with(AOFF, 4, 2, (uint64_t)4); broken("a term's alternatives do not tile it", rq);
        rq = base(); rq.term_offsets = with(TOFF, 4, 0, (uint64_t)1); broken("the terms start at 1", rq);
        rq = base(); rq.seed_offsets = with(rq.seed_offsets, 4, 0, (uint64_t)1); broken("the queries start at 1", rq);
        rq = base(); rq.seed_offsets = with(rq.seed_offsets, 4, 3, (uint64_t)nq - 1); broken("the queries end before the last", rq);
        rq = base(); rq.seed_offsets = with(rq.seed_offsets, 4, 3, (uint64_t)nq + 1); broken("the queries end behind the last", rq);
        rq = base(); rq.seed_offsets = with(rq.seed_offsets, 4, 2, (uint64_t)1); broken("the queries decrease", rq);
        // every query's alternative belongs to its term
        rq = base(); rq.any_query_alt = with(rq.any_query_alt, nq, nq - 1, (uint32_t)1); broken("a query of the last term in the first term's alternative", rq);
        rq = base(); rq.any_query_alt = with(rq.any_query_alt, nq, 0, (uint32_t)2); broken("a query of the first term in the last term's alternative", rq);
        rq = base(); rq.any_query_alt = with(rq.any_query_alt, nq, 0, (uint32_t)3); broken("a query in an alternative that is none", rq);
        rq = base(); rq.any_query_alt = with(rq.any_query_alt, nq, 0, 0xffffffffu); broken("a query in alternative 2^32 - 1", rq);
        // seed_pos + query length <= alternative length
        rq = base(); rq.seed_pos = with(rq.seed_pos, nq, nq - 1, (uint32_t)1); broken("a query that ends behind its alternative", rq);
        rq = base(); rq.seed_pos = with(rq.seed_pos, nq, 0, 0xffffffffu); broken("a position of 2^32 - 1", rq);
        rq = base(); rq.qoffsets = with(rq.qoffsets, nq + 1, nq, (uint64_t)100); broken("a query longer than its alternative", rq);
    }
    {   // in exact bytes a query IS its alternative; under fold it may be a part of it
        static const uint64_t QOFF[] = {0, 1, 4, 6};
        static const uint32_t POS[] = {1, 0, 0};
        SearchRequest rq = exact_rq();
        rq.qoffsets = QOFF;
        rq.seed_pos = POS;
        broken("exact: a query that is a part of its alternative", rq);
        rq.any_fold = true;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "fold: a query that is a part of its alternative");
    }
    {   // one member of the block on a batch that is none
        SearchRequest rq;
        rq.qbytes = TERMS;
        rq.qoffsets = X_QOFF;
        rq.nq = 3;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "plain");
        rq.any_fold = true;
        broken("any_fold on a plain batch", rq);
        rq.any_fold = false;
        rq.any_nalts = 1;
        broken("any_nalts on a plain batch", rq);
        rq.any_nalts = 0;
        rq.any_query_alt = X_QALT;
        broken("any_query_alt on a plain batch", rq);
    }
    {   // an empty batch and a batch whose sets are all void
        static const uint64_t ZERO[] = {0, 0, 0};
        SearchRequest rq;
        rq.qbytes = TERMS; rq.qoffsets = ZERO; rq.nq = 0;
        rq.group_offsets = ZERO; rq.ngroups = 0; rq.exclude = Z8;
        rq.term_bytes = TERMS; rq.term_offsets = ZERO; rq.nterms = 0;
        rq.seed_offsets = ZERO; rq.seed_pos = X_POS;
        rq.any_term_alts = ZERO; rq.any_alt_offsets = ZERO; rq.any_query_alt = X_QALT;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "no set");
        static const uint64_t ID2[] = {0, 1, 2};
        rq.group_offsets = ID2; rq.ngroups = 2; rq.nterms = 2;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "two void sets");
    }
}

static void shape()
{
    for (bool fold : {false, true}) {
        const SearchRequest rq = fold ? fold_rq() : exact_rq();
        const BatchShape b(rq, 2, rq.qoffsets[rq.nq], false, false, false);
        CHECK(b.any && b.any_fold == fold && b.seeded && b.terms && !b.near && !b.edits && !b.fold_near && !b.seq && !b.seqc && !b.regex &&
                  !b.sa_order && !b.fused_ok && !b.resident_ok && !b.mid_ok,
              "shape, fold %d", (int)fold);
        CHECK(b.nrow == 3 && b.nterm == 3 && b.nvq == 2ull * rq.nq && b.ntp == 6 && b.nrp == 6, "pair spaces, fold %d", (int)fold);
    }
    SearchRequest plain;
    plain.qbytes = TERMS;
    plain.qoffsets = X_QOFF;
    plain.nq = 3;
    const BatchShape p(plain, 2, 7, false, false, false);
    CHECK(!p.any && !p.any_fold, "a plain batch is no any-of batch");
}

static size_t up(size_t x) { return (x + 63) / 64 * 64; }

// The block, restated: 24 bytes of pointers, (nterm + 1) and (nalts + 1) u64, nq u32, every region on a multiple of 64;
// behind the hits of a seeded layout, on the next multiple of 64; and nothing at all in any other batch.
static void layout()
{
    for (uint32_t nterm : {0u, 1u, 7u, 8u, 63u, 64u, 65u})
        for (uint32_t nalts : {0u, 1u, 7u, 8u, 64u, 4095u})
            for (uint32_t nq : {0u, 1u, 15u, 16u, 17u, 4096u}) {
                const AnyBlock A(true, nterm, nalts, nq);
                const size_t talts = 64, aoff = talts + up(((size_t)nterm + 1) * 8), qalt = aoff + up(((size_t)nalts + 1) * 8),
                             end = qalt + up((size_t)nq * 4);
                CHECK(A.hdr == 0 && A.talts == talts && A.aoff == aoff && A.qalt == qalt && A.end == end, "AnyBlock %u %u %u", nterm, nalts, nq);
                const AnyBlock none(false, nterm, nalts, nq);
                CHECK(none.hdr == 0 && none.talts == 0 && none.aoff == 0 && none.qalt == 0 && none.end == 0, "no block %u %u %u", nterm, nalts, nq);
                for (uint64_t nc : {1ull, 3ull, 5ull}) {
                    const uint64_t ntp = nterm * nc, nrp = nterm * nc, total = 3ull * nalts + 1;
                    const SeedLayout near_like(nterm, nterm, nq, total, ntp, nrp, true, ClassBlock());
                    const SeedLayout S(nterm, nterm, nq, total, ntp, nrp, true, ClassBlock(), RegexBlock(), A);
                    const SeedLayout T(nterm, nterm, nq, total, ntp, nrp, true, ClassBlock(), RegexBlock(), none);
                    CHECK(near_like.any == near_like.end && T.end == near_like.end && T.any == T.end, "no block moves nothing");
                    CHECK(S.goff == near_like.goff && S.soff == near_like.soff && S.foff == near_like.foff && S.over == near_like.over &&
                              S.pos == near_like.pos && S.fvoid == near_like.fvoid && S.tflags == near_like.tflags &&
                              S.budget == near_like.budget && S.fbytes == near_like.fbytes && S.tcnt == near_like.tcnt &&
                              S.gdrv == near_like.gdrv && S.cnt == near_like.cnt,
                          "the block moves no region %u %u %u", nterm, nalts, nq);
                    CHECK(S.any == up(near_like.end) && S.end == S.any + end && S.any % 64 == 0 && S.any >= S.cnt + nrp * 4,
                          "the block's place %u %u %u", nterm, nalts, nq);
                    CHECK(S.over + 8 <= S.pos, "room for the overflow word");
                }
            }
    CHECK(sizeof(void *) * 3 <= 64, "the pointers fit their region");
}

static std::vector<std::string> norm(std::vector<std::string> in, bool fold)
{
    std::string bytes;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &s : in) {
        bytes += s;
        off.push_back(bytes.size());
    }
    bytes.push_back('\0');
    return any_normalise(reinterpret_cast<const uint8_t *>(bytes.data()), off.data(), 0, in.size(), fold).alts;
}

static void normalisation()
{
    using V = std::vector<std::string>;
    CHECK(norm({"warn", "error", "errors", "warn", "Fatal"}, false) == V({"Fatal", "error", "warn"}), "duplicates, a superstring, the sort");
    CHECK(norm({"warn", "WARN", "Error"}, true) == V({"error", "warn"}), "the fold");
    CHECK(norm({"a\nb", "c"}, false) == V({"c"}) && norm({"\n", "x\n"}, false).empty(), "the newline rule");
    CHECK(norm({"@", "`", "\xc9", "\xe9", "[", "{"}, true) == V({"@", "[", "`", "{", "\xc9", "\xe9"}), "what does not fold");
    CHECK(norm({"abc", "bcd", "abcd", "xbc"}, false) == V({"abc", "bcd", "xbc"}), "overlaps stay, the string that holds one goes");
    CHECK(norm({std::string("a\0", 2), "a"}, false) == V({"a"}) && norm({std::string("b\0", 2), std::string("\0", 1) + "c"}, false).size() == 2, "0x00 is a byte");
    CHECK(norm({"\xff", "\x7f", "\x80"}, false) == V({"\x7f", "\x80", "\xff"}), "unsigned order");
    const uint32_t want[] = {6, 5, 4, 4, 3, 3, 3, 3, 2};
    for (uint32_t n = 1; n <= 9; ++n) CHECK(any_seed_letters(n, 6) == want[n - 1], "letters of %u", n);
    CHECK(any_seed_letters(16, 6) == 2 && any_seed_letters(17, 6) == 1 && any_seed_letters(32, 6) == 1 && any_seed_letters(32, 1) == 1 &&
              any_seed_letters(1, 5) == 5 && any_seed_letters(3, 2) == 2 && any_seed_letters(0, 5) == 5,
          "letters at the caps");
    for (uint32_t n = 1; n <= ANY_MAX_ALTS_FOLD; ++n) CHECK(any_seed_letters(n, 6) >= 1 && (n << any_seed_letters(n, 6)) <= 64, "64 queries, %u", n);
}

int main()
{
    rules();
    shape();
    layout();
    normalisation();
    if (failures) {
        std::printf("any_request: %d FAILED\n", failures);
        return 1;
    }
    std::printf("any_request: ok\n");
    return 0;
}
