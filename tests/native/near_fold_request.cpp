// near_fold_request.cpp -- the request rule of a batch within a budget UNDER FOLD (csrc/search_layout.h, near_fold;
// DESIGN.md 4.19) on the CPU: one valid request of each kind, every new clause broken, what BatchShape makes of the flag,
// and that the flag asks nothing of SeedLayout -- a fold-near batch carves what a near batch carves.  Header only: no
// library, no device.  (tests/test_near_icase_host.py builds it with g++ under AddressSanitizer + UBSan.)
#include <cstdio>
#include <cstring>
#include <initializer_list>

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

// three patterns `abc`, `De`, `f1`, budgets 1, 0, 1: piece by piece the spellings of a seed of at most one letter
static const uint8_t QUERIES[] = "ABabCcDdEeFf1";                                   // a | bc -> `a`: A a, `b`: B b ... (bytes only: the rule reads none)
static const uint64_t QOFF[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13};       // 13 queries of a byte each
static const uint8_t TERMS[] = "abcdef1";
static const uint64_t TOFF[] = {0, 3, 5, 7};
static const uint64_t SOFF[] = {0, 4, 6, 13};
static const uint32_t POS[13] = {0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1};
static const uint64_t IDENT[] = {0, 1, 2, 3};
static const uint8_t BUDGET[] = {1, 0, 1}, NO_EXCLUDE[] = {0, 0, 0}, ONE_EXCLUDES[] = {0, 1, 0}, Z8[8] = {0};
static const uint64_t SEGS[] = {0, 1, 2, 3}, CLS_GROUPS[] = {0, 1, 2, 3};
static const uint32_t CORES[] = {0, 1, 0, 1, 0, 1};

static SearchRequest fold_near_rq()
{
    SearchRequest rq;
    rq.qbytes = QUERIES;
    rq.qoffsets = QOFF;
    rq.nq = 13;
    rq.group_offsets = IDENT;
    rq.ngroups = 3;
    rq.exclude = NO_EXCLUDE;
    rq.term_bytes = TERMS;
    rq.term_offsets = TOFF;
    rq.nterms = 3;
    rq.seed_offsets = SOFF;
    rq.seed_pos = POS;
    rq.near_budget = BUDGET;
    rq.near_fold = true;
    return rq;
}

static SearchRequest fold_edit_rq()
{
    SearchRequest rq = fold_near_rq();
    rq.near_edits = true;
    return rq;
}

static void class_block(SearchRequest &r)
{
    r.class_bytes = TERMS;
    r.class_plane = Z8;
    r.class_offsets = SEGS;
    r.class_nsegs = 3;
    r.class_groups = CLS_GROUPS;
    r.class_cores = CORES;
    r.class_void = Z8;
}

int main()
{
    for (const bool edits : {false, true}) {
        const SearchRequest valid = edits ? fold_edit_rq() : fold_near_rq();
        const char *what = edits ? "fold edit" : "fold near";
        for (SearchMode mode : {SEARCH_FULL, SEARCH_COUNTS, SEARCH_IDS}) {
            SearchRequest rq = valid;
            rq.mode = mode;
            CHECK(check_request(rq, 2, true) == REQUEST_OK && seeded_request_ok(rq), "%s, mode %d", what, (int)mode);
        }
        // what the driver reads off it
        const BatchShape s(valid, 2, 13, false, false, false);
        CHECK(s.seeded && s.near && s.fold_near && s.edits == edits && !s.seq && !s.seqc && s.nterm == 3 && s.nrow == 3 && s.nvq == 26 &&
                  s.ntp == 6 && s.nrp == 6 && !s.fused_ok && !s.mid_ok && !s.resident_ok,
              "%s: shape", what);
        SearchRequest exact = valid;
        exact.near_fold = false;
        const BatchShape e(exact, 2, 13, false, false, false);
        CHECK(e.near && !e.fold_near && e.edits == edits && check_request(exact, 2, true) == REQUEST_OK, "%s without the flag", what);

        // every new clause broken
        SearchRequest rq = valid;
        rq.near_budget = nullptr;                       // near_fold without budgets
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED && !seeded_request_ok(rq), "%s without budgets", what);
        rq = valid;
        rq.seq_anchors = Z8;                            // with sequence anchors, beside the flags and in their place
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED && !seeded_request_ok(rq), "%s with seq_anchors", what);
        rq.exclude = nullptr;
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED && !seeded_request_ok(rq), "%s with seq_anchors alone", what);
        rq = valid;
        rq.exclude = ONE_EXCLUDES;                      // with a term that excludes
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED && !seeded_request_ok(rq), "%s with exclude", what);
        rq.near_fold = false;                           // (the exact-byte batch leaves the flags to its caller, as before)
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "%s: exclude flags without the flag", what);
        rq = valid;
        class_block(rq);                                // with a class block
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED && !seeded_request_ok(rq), "%s with a class block", what);
        rq = valid;
        rq.mode = SEARCH_DEVICE;                        // (the all-terms rule is judged first and says so)
        CHECK(check_request(rq, 2, true) == REQUEST_ALL_TERMS, "%s to a device result", what);
    }
    {   // the flag alone, on a plain batch and on a batch under fold without budgets
        SearchRequest rq;
        rq.qbytes = QUERIES;
        rq.qoffsets = QOFF;
        rq.nq = 13;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "plain");
        rq.near_fold = true;
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED, "near_fold on a plain batch");
        const BatchShape s(rq, 2, 13, false, false, false);
        CHECK(!s.near && !s.fold_near, "near_fold without a seeded batch says nothing");
    }
    // no new region: the sizes of a seeded layout with near = true are what they are today, written out
    for (const uint32_t n : {1u, 3u, 63u, 64u, 65u}) {
        const uint32_t nq = n * 64, nc = 5;
        const uint64_t ttotal = (uint64_t)n * 11, ntp = (uint64_t)n * nc, nrp = ntp;
        const SeedLayout S(n, n, nq, ttotal, ntp, nrp, true, ClassBlock());
        auto up = [](size_t x) { return (x + 63) / 64 * 64; };
        size_t o = 0;
        const size_t goff = o;      o = up(o + ((size_t)n + 1) * 8);
        const size_t soff = o;      o = up(o + ((size_t)n + 1) * 8);
        const size_t foff = o;      o = up(o + ((size_t)n + 1) * 8);
        const size_t over = o;      o = up(o + 64);
        const size_t pos = o;       o = up(o + (size_t)nq * 4);
        const size_t fvoid = o;     o = up(o + n);
        const size_t tflags = o;    o = up(o + n);
        const size_t budget = o;    o = up(o + n);
        const size_t anchors = o;   o = up(o + 0);
        const size_t fbytes = o;    o = up(o + (size_t)ttotal + 32);
        const size_t tcnt = o;      o = up(o + (size_t)ntp * 4);
        const size_t gdrv = o, cnt = gdrv + (size_t)nrp * 4, end = cnt + (size_t)nrp * 4;
        CHECK(S.goff == goff && S.soff == soff && S.foff == foff && S.over == over && S.pos == pos && S.fvoid == fvoid &&
                  S.tflags == tflags && S.budget == budget && S.anchors == anchors && S.fbytes == fbytes && S.tcnt == tcnt &&
                  S.gdrv == gdrv && S.cnt == cnt && S.end == end,
              "SeedLayout of %u patterns with 64 queries each", n);
    }
    if (failures) {
        std::printf("near_fold_request: %d check(s) FAILED\n", failures);
        return 1;
    }
    std::printf("near_fold_request: ok\n");
    return 0;
}
