// The request rules, the route rules and the layouts of a search batch (csrc/search_layout.h) checked on the CPU.
//   1. Every layout restated as a table of region sizes: every start, the 64-byte rounding, no overlap, and end == the
//      reservation the driver made before the header existed (the old formulas written out), at 1, 63, 64, 65 and
//      2^20 + 1 rows / terms / queries, 1 and 5 chunks, term bytes of 1, 31, 32, 33 and 96, with and without budgets,
//      sequence anchors and a class block of 0, 1 and 255 sets over 0 and 33 positions.
//   2. Every route rule on both sides of its edge, the answers written down as numbers.
//   3. One valid request of every kind, and for every clause of every rule the same request with that clause broken.
// Exit code 0 and "search_layout: ok" = every check holds.  Built by tests/test_host.py with g++
// -fsanitize=address,undefined against search_layout.h alone.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "search_layout.h"

using namespace pss;

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("search_layout.cpp:%d: %s  [", __LINE__, #cond);        \
            printf(__VA_ARGS__);                                           \
            printf("]\n");                                                 \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static size_t up(size_t x) { return (x + 63) / 64 * 64; }

// Regions of `sizes` one behind the other on multiples of 64; the regions of `tail` follow back to back, unrounded.
// got: the layout's offsets in the same order, its end last.
static void table(const char *what, const std::vector<size_t> &sizes, const std::vector<size_t> &tail, const std::vector<size_t> &got)
{
    CHECK(got.size() == sizes.size() + tail.size() + 1, "%s", what);
    size_t at = 0, r = 0;
    for (size_t k = 0; k < sizes.size(); ++k, ++r) {
        CHECK(got[r] == at, "%s region %zu: %zu, not %zu", what, r, got[r], at);
        CHECK(at % 64 == 0, "%s region %zu", what, r);
        at = up(at + sizes[k]);
        CHECK(got[r] + sizes[k] <= got[r + 1], "%s region %zu overlaps the next", what, r);
    }
    for (size_t k = 0; k < tail.size(); ++k, ++r) {
        CHECK(got[r] == at, "%s tail %zu: %zu, not %zu", what, r, got[r], at);
        at += tail[k];
    }
    CHECK(got[r] == at, "%s end: %zu, not %zu", what, got[r], at);
}

static const uint32_t COUNTS[] = {1, 63, 64, 65, (1u << 20) + 1};
static const uint32_t CHUNKS[] = {1, 5};
static const uint64_t TERM_BYTES[] = {1, 31, 32, 33, 96};

struct Block {
    bool seq, seqc;
    uint32_t nsegs, nsets;
    uint64_t total;
};
static std::vector<Block> blocks(uint32_t nterms)
{
    std::vector<Block> b = {{false, false, 0, 0, 0}, {true, false, 0, 0, 0}};
    for (uint32_t nsets : {0u, 1u, 255u})
        for (uint64_t total : {(uint64_t)0, (uint64_t)33}) b.push_back({true, true, nterms, nsets, total});
    return b;
}

// anchor_room() as it stood
static size_t old_anchor_room(const Block &b, uint32_t nrow)
{
    if (!b.seq) return 0;
    size_t room = up(nrow);
    if (b.seqc)
        room += up(((size_t)b.nsegs + 1) * 8) + up(((size_t)nrow + 1) * 8) + up((size_t)b.nsegs * 8) + up((size_t)b.nsets * 32) +
                2 * up(b.total + 32);
    return room;
}

static void class_block(const Block &b, uint32_t nrow)
{
    const ClassBlock L(b.seq, b.seqc, nrow, b.nsegs, b.total, b.nsets);
    CHECK(L.end == old_anchor_room(b, nrow), "%d %d %u", b.seq, b.seqc, nrow);
    if (!b.seq) {
        CHECK(L.anchors == 0 && L.end == 0, "no block");
        return;
    }
    if (!b.seqc) {
        table("ClassBlock (anchors alone)", {nrow}, {}, {L.anchors, L.end});
        return;
    }
    const size_t ns = b.nsegs;
    table("ClassBlock", {nrow, (ns + 1) * 8, ((size_t)nrow + 1) * 8, ns * 8, (size_t)b.nsets * 32, (size_t)b.total + 32, (size_t)b.total + 32}, {},
          {L.anchors, L.seg_off, L.seg_goff, L.cores, L.sets, L.bytes, L.plane, L.end});
    // the 32 zero bytes behind the bytes and behind the plane are inside their regions
    CHECK(L.plane - L.bytes >= b.total + 32 && L.end - L.plane >= b.total + 32, "zero bytes behind the class bytes and the plane");
}

static void layouts()
{
    for (uint32_t nrow : COUNTS)
        for (uint32_t nq : COUNTS)
            for (uint32_t nc : CHUNKS)
                for (const Block &b : blocks(nq)) {
                    class_block(b, nrow);
                    const uint64_t nrp = (uint64_t)nrow * nc;
                    const ClassBlock C(b.seq, b.seqc, nrow, b.nsegs, b.total, b.nsets);
                    // pick_drivers: goff_room + flag_room + anch_room + nrp * 12
                    const TermsLayout T(nrow, nq, nrp, C);
                    table("TermsLayout", {((size_t)nrow + 1) * 8, nq, C.end}, {(size_t)nrp * 4, (size_t)nrp * 4, (size_t)nrp * 4},
                          {T.goff, T.tflags, T.anchors, T.gdrv, T.lo, T.cnt, T.end});
                    CHECK(T.end == up(((size_t)nrow + 1) * 8) + up(nq) + old_anchor_room(b, nrow) + (size_t)nrp * 12, "%u %u %u", nrow, nq, nc);
                    CHECK(T.cls.end == C.end && T.cls.plane == C.plane, "the embedded block");
                    // seed_drivers: nq seed queries of nterm terms
                    for (uint32_t nterm : COUNTS)
                        for (uint64_t ttotal : TERM_BYTES)
                            for (bool near : {false, true}) {
                                if (near && (b.seq || nterm != nrow)) continue;     // (budgets: identity groups, no sequence)
                                if (b.seqc) {
                                    if (nterm != nq) continue;                      // (blocks(nq) sized the segments for nq cores)
                                }
                                const uint64_t ntp = (uint64_t)nterm * nc;
                                const SeedLayout S(nrow, nterm, nq, ttotal, ntp, nrp, near, C);
                                table("SeedLayout",
                                      {((size_t)nrow + 1) * 8, ((size_t)nterm + 1) * 8, ((size_t)nterm + 1) * 8, near ? (size_t)64 : 0, (size_t)nq * 4,
                                       nterm, nterm, near ? (size_t)nterm : 0, C.end, (size_t)ttotal + 32, (size_t)ntp * 4},
                                      {(size_t)nrp * 4, (size_t)nrp * 4},
                                      {S.goff, S.soff, S.foff, S.over, S.pos, S.fvoid, S.tflags, S.budget, S.anchors, S.fbytes, S.tcnt, S.gdrv,
                                       S.cnt, S.end});
                                const size_t goff_room = up(((size_t)nrow + 1) * 8), toff_room = up(((size_t)nterm + 1) * 8);
                                const size_t over_room = near ? 64 : 0, pos_room = up((size_t)nq * 4), flag_room = up(nterm);
                                const size_t budget_room = near ? flag_room : 0, anch_room = old_anchor_room(b, nrow);
                                const size_t byte_room = up(ttotal + 32), tcnt_room = up((size_t)ntp * 4);
                                CHECK(S.end == goff_room + 2 * toff_room + over_room + pos_room + 2 * flag_room + budget_room + anch_room +
                                                   byte_room + tcnt_room + (size_t)nrp * 8,
                                      "%u %u %u %llu %d", nrow, nterm, nq, (unsigned long long)ttotal, near);
                                CHECK(S.tcnt - S.fbytes >= ttotal + 32, "zero bytes behind the terms");
                                if (near) CHECK(S.pos - S.over >= 8 && S.anchors - S.budget >= nterm, "overflow word and budgets");
                            }
                    // Q_ANCHOR: round_up(nq, 64) + nvq
                    const uint64_t nvq = (uint64_t)nq * nc;
                    const AnchorFlags A(nq, nvq);
                    table("AnchorFlags", {nq}, {(size_t)nvq}, {A.flags, A.edge, A.end});
                    CHECK(A.end == up(nq) + nvq, "%u %u", nq, nc);
                }
    // pinned: two ends written down
    CHECK(TermsLayout(65, 64, 65, ClassBlock(true, false, 65, 0, 0, 0)).end == 576 + 64 + 128 + 780, "TermsLayout 65 64");
    CHECK(SeedLayout(64, 64, 65, 33, 64, 64, true, ClassBlock()).end == 576 + 2 * 576 + 64 + 320 + 2 * 64 + 64 + 0 + 128 + 256 + 512,
          "SeedLayout 64 64 65 33 near");
    CHECK(ClassBlock(true, true, 1, 1, 33, 255).end == 64 + 64 + 64 + 64 + 8192 + 128 + 128, "ClassBlock 1 1 33 255");

    // Q_SMALL and the pinned words
    CHECK(SmallWords::PARTIAL == 0 && SmallWords::TOTAL == 1024 && SmallWords::MID_STATE == 1032 && SmallWords::BYTES == 8448, "Q_SMALL");
    CHECK(SmallWords::MID_STATE * 8 + 32 <= SmallWords::BYTES && SEARCH_SCAN_BLOCKS == 1024, "MidState (32 bytes) fits");
    CHECK(PW_COUNT == 0 && PW_BYTES == 1 && PW_NEAR_OVERFLOW == 2, "pinned words");
}

static void staging()
{
    // the query staging: q_room = round_up(qtotal + 32, 64), o_room = round_up(off_bytes, 64);
    // staged = anchored ? q_room + o_room + nq : qtotal + 32 + off_bytes + 64
    for (uint32_t nq : COUNTS)
        for (uint64_t qtotal : TERM_BYTES)
            for (bool anchored : {false, true}) {
                const size_t off_bytes = ((size_t)nq + 1) * 8, q_room = up(qtotal + 32), o_room = up(off_bytes);
                const QueryStage Q(anchored, nq, qtotal, off_bytes);
                table("QueryStage", {(size_t)qtotal + 32, off_bytes}, {}, {Q.q, Q.off, Q.flags});
                CHECK(Q.staged == (anchored ? q_room + o_room + nq : qtotal + 32 + off_bytes + 64), "%u %llu %d", nq, (unsigned long long)qtotal, anchored);
                CHECK(Q.own_flags == q_room && Q.own_bytes == q_room + nq, "the vectors of an anchored batch");
                CHECK(Q.fits() == (nq <= 65), "all but the 8 MiB of offsets of 2^20 + 1 queries fit");
            }
    CHECK(QueryStage::TINY_Q == 32768 && QueryStage::TINY_OFF == 32768 + 8192 && SM_QUERY_ROOM == 8192, "the tiny staging");
    CHECK(SEARCH_STAGE_Q == 2097152 && SEARCH_STAGE_R == 4194304, "the staging sizes");
    // staged bytes at kStageQ and one more: plain, qtotal + 32 + 16 + 64 = 2097152 <=> qtotal = 2097040
    CHECK(QueryStage(false, 1, 2097040, 16).staged == 2097152 && QueryStage(false, 1, 2097040, 16).fits(), "plain, on the edge");
    CHECK(QueryStage(false, 1, 2097041, 16).staged == 2097153 && !QueryStage(false, 1, 2097041, 16).fits(), "plain, one more");
    // anchored, nq = 64: q_room + 576 + 64 = 2097152 <=> q_room = 2096512 <=> qtotal + 32 in (2096448, 2096512]
    CHECK(QueryStage(true, 64, 2096480, 520).staged == 2097152 && QueryStage(true, 64, 2096480, 520).fits(), "anchored, on the edge");
    CHECK(QueryStage(true, 64, 2096481, 520).staged == 2097216 && !QueryStage(true, 64, 2096481, 520).fits(), "anchored, one more");
    CHECK(QueryStage(true, 65, 2096480, 528).staged == 2097153 && !QueryStage(true, 65, 2096480, 528).fits(), "anchored, one more flag");

    // the result staging: round_up(E * 8, 64) + round_up(B, 64) + nrow * 8 <= kStageR
    for (uint32_t nrow : COUNTS)
        for (uint64_t E : {(uint64_t)0, (uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)65})
            for (uint64_t B : TERM_BYTES) {
                const ResultStage R(E, B, nrow);
                table("ResultStage", {(size_t)E * 8, (size_t)B}, {(size_t)nrow * 8}, {R.offsets, R.bytes, R.counts, R.end});
                CHECK(R.end == up(E * 8) + up(B) + (size_t)nrow * 8, "%u", nrow);
            }
    // E = 8: 64 bytes of offsets; nrow = 8: 64 bytes of counts; B = 4194304 - 128 on the edge, one more byte rounds up past it
    CHECK(ResultStage(8, 4194176, 8).end == 4194304 && ResultStage(8, 4194176, 8).fits(), "result, on the edge");
    CHECK(ResultStage(8, 4194177, 8).end == 4194368 && !ResultStage(8, 4194177, 8).fits(), "result, one more byte");
    CHECK(ResultStage(8, 4194176, 9).end == 4194312 && !ResultStage(8, 4194176, 9).fits(), "result, one more row");
}

// ---- the route rules -----------------------------------------------------------------------------------------------

struct Plain {      // nq patterns of plen bytes each
    std::vector<uint64_t> off;
    SearchRequest rq;
    Plain(uint32_t nq, uint64_t plen) : off((size_t)nq + 1)
    {
        for (uint32_t i = 0; i <= nq; ++i) off[i] = i * plen;
        rq.qbytes = reinterpret_cast<const uint8_t *>("");
        rq.qoffsets = off.data();
        rq.nq = nq;
    }
    uint64_t total() const { return off.back(); }
};

static BatchShape shape(const SearchRequest &rq, uint32_t nc, uint64_t qtotal, bool s = false, bool b = false, bool m = false)
{
    return BatchShape(rq, nc, qtotal, s, b, m);
}

static void routes()
{
    CHECK(SM_MAX_VQ == 1024 && SM_MAX_PLEN == 256 && SM_BLOCK_MAX_VQ == 64 && MID_MAX == 65536 && SM_OFF_QUERY == 32768, "the constants");
    static const uint8_t some[4] = {1, 1, 1, 1};
    static const uint64_t goff[2] = {0, 1};
    {   // qtotal + 32 at 8192 and 8193 (32 patterns of 255 bytes: 8160)
        Plain p(32, 255);
        const BatchShape a = shape(p.rq, 1, 8160), b = shape(p.rq, 1, 8161);
        CHECK(p.total() == 8160 && a.tiny && a.fused_ok && !b.tiny && !b.fused_ok && b.mid_ok, "qtotal + 32 = 8192 | 8193");
        CHECK(a.nvq == 32 && a.nrp == 32 && a.nrow == 32 && a.nterm == 0 && a.ntp == 0 && a.off_bytes == 264, "the counts");
    }
    {   // nq at 1023 and 1024: the offsets take 8192 and 8200 bytes
        Plain p(1023, 1), q(1024, 1);
        const BatchShape a = shape(p.rq, 1, 1023), b = shape(q.rq, 1, 1024);
        CHECK(a.off_bytes == 8192 && a.tiny && a.fused_ok, "nq = 1023");
        CHECK(b.off_bytes == 8200 && !b.tiny && !b.fused_ok && b.mid_ok, "nq = 1024");
    }
    {   // nvq at SM_MAX_VQ and one more: 512 x 2 chunks, 342 x 3 = 1026, 1023 x 1 + ...: 205 x 5 = 1025
        Plain p(512, 1), q(205, 1);
        CHECK(shape(p.rq, 2, 512).nvq == 1024 && shape(p.rq, 2, 512).fused_ok, "nvq = 1024");
        CHECK(shape(q.rq, 5, 205).nvq == 1025 && shape(q.rq, 5, 205).tiny && !shape(q.rq, 5, 205).fused_ok, "nvq = 1025");
    }
    {   // a pattern of 256 and of 257 bytes
        Plain p(2, 256), q(2, 257);
        CHECK(shape(p.rq, 1, 512).fused_ok && !shape(q.rq, 1, 514).fused_ok && shape(q.rq, 1, 514).tiny, "SM_MAX_PLEN");
        q.off[1] = 1;       // (the second pattern alone is too long: 1 and 513 bytes)
        CHECK(!shape(q.rq, 1, 514).fused_ok, "the longest pattern decides");
    }
    {   // the resident route: one query, low latency, nvq at 64 and 65
        Plain p(1, 8);
        p.rq.low_latency = true;
        CHECK(shape(p.rq, 64, 8).resident_ok && shape(p.rq, 64, 8).nvq == 64, "nvq = 64");
        CHECK(!shape(p.rq, 65, 8).resident_ok && shape(p.rq, 65, 8).fused_ok, "nvq = 65");
        CHECK(!shape(p.rq, 1, 8, false, true).resident_ok && shape(p.rq, 1, 8, false, true).fused_ok, "no_block_path");
        CHECK(!shape(p.rq, 1, 8, true).resident_ok && !shape(p.rq, 1, 8, true).fused_ok && shape(p.rq, 1, 8, true).mid_ok, "no_small_path");
        p.rq.low_latency = false;
        CHECK(!shape(p.rq, 1, 8).resident_ok && shape(p.rq, 1, 8).fused_ok, "not asked for");
        Plain two(2, 8);
        two.rq.low_latency = true;
        CHECK(!shape(two.rq, 1, 16).resident_ok && shape(two.rq, 1, 16).fused_ok, "two queries");
    }
    {   // nvq at MID_MAX and one more
        Plain p(65536, 1), q(65537, 1), r(13108, 1);
        CHECK(shape(p.rq, 1, 65536).mid_ok && !shape(q.rq, 1, 65537).mid_ok, "nvq = 65536 | 65537");
        CHECK(shape(r.rq, 5, 13108).nvq == 65540 && !shape(r.rq, 5, 13108).mid_ok, "five chunks");
        CHECK(!shape(p.rq, 1, 65536, false, false, true).mid_ok, "no_mid_pipeline");
        CHECK(!shape(p.rq, 1, 65536).fused_ok && !shape(p.rq, 1, 65536).tiny, "not tiny");
    }
    {   // each mode
        Plain p(3, 4);
        struct { SearchMode mode; bool counts, device, ids, fused, mid; } want[] = {
            {SEARCH_FULL, false, false, false, true, true}, {SEARCH_COUNTS, true, false, false, false, false},
            {SEARCH_DEVICE, false, true, false, false, true}, {SEARCH_IDS, false, false, true, false, false}};
        for (const auto &w : want) {
            p.rq.mode = w.mode;
            const BatchShape s = shape(p.rq, 2, 12);
            CHECK(s.counts == w.counts && s.device == w.device && s.ids == w.ids && s.fused_ok == w.fused && s.mid_ok == w.mid && s.tiny, "mode %d", (int)w.mode);
            CHECK(!s.anchored && !s.terms && !s.seq && !s.seqc && !s.seeded && !s.near && !s.edits && !s.sa_order, "mode %d", (int)w.mode);
        }
    }
    {   // sa_order: kept by a plain batch, which then takes the general pipeline; suppressed by counts, anchors and groups
        Plain p(1, 4);
        p.rq.sa_order = true;
        CHECK(shape(p.rq, 1, 4).sa_order && !shape(p.rq, 1, 4).fused_ok && !shape(p.rq, 1, 4).mid_ok && shape(p.rq, 1, 4).tiny, "sa_order");
        p.rq.mode = SEARCH_IDS;
        CHECK(shape(p.rq, 1, 4).sa_order, "ids keep it");
        p.rq.mode = SEARCH_COUNTS;
        CHECK(!shape(p.rq, 1, 4).sa_order, "counts");
        p.rq.mode = SEARCH_FULL;
        p.rq.anchors = some;
        const BatchShape a = shape(p.rq, 1, 6);
        CHECK(!a.sa_order && a.anchored && !a.tiny && !a.fused_ok && !a.mid_ok, "anchors");
        p.rq.anchors = nullptr;
        p.rq.group_offsets = goff;
        p.rq.ngroups = 1;
        p.rq.exclude = some;
        const BatchShape t = shape(p.rq, 1, 4);
        CHECK(!t.sa_order && t.terms && !t.seq && !t.seeded && t.tiny && !t.fused_ok && !t.mid_ok, "groups");
    }
    {   // the kinds of group batch, and their counts: 3 seed queries of 2 terms in 1 group over 5 chunks
        static const uint64_t g1[2] = {0, 2}, toff[3] = {0, 3, 6}, soff[3] = {0, 1, 3};
        static const uint32_t pos[3] = {0, 0, 0};
        Plain p(3, 2);
        p.rq.group_offsets = g1;
        p.rq.ngroups = 1;
        p.rq.seq_anchors = some;
        BatchShape s = shape(p.rq, 5, 6);
        CHECK(s.terms && s.seq && !s.seqc && !s.seeded && s.nrow == 1 && s.nrp == 5 && s.nvq == 15 && s.nterm == 0 && s.ntp == 0, "sequence");
        p.rq.class_bytes = some;
        s = shape(p.rq, 5, 6);
        CHECK(s.seq && s.seqc, "class");
        p.rq.class_bytes = nullptr;
        p.rq.term_bytes = some;
        p.rq.term_offsets = toff;
        p.rq.nterms = 2;
        p.rq.seed_offsets = soff;
        p.rq.seed_pos = pos;
        s = shape(p.rq, 5, 6);
        CHECK(s.seeded && s.seq && !s.near && !s.edits && s.nterm == 2 && s.ntp == 10 && s.nrow == 1 && s.nrp == 5 && s.nvq == 15, "seeded");
        p.rq.seq_anchors = nullptr;
        p.rq.exclude = some;
        p.rq.near_edits = true;     // (without budgets it says nothing)
        s = shape(p.rq, 5, 6);
        CHECK(s.seeded && !s.seq && !s.near && !s.edits, "edits without budgets");
        p.rq.near_budget = some;
        s = shape(p.rq, 5, 6);
        CHECK(s.near && s.edits, "edits");
        p.rq.near_edits = false;
        s = shape(p.rq, 5, 6);
        CHECK(s.near && !s.edits, "near");
    }
}

// ---- the request rules ---------------------------------------------------------------------------------------------

static const uint8_t B8[8] = {1, 1, 1, 1, 1, 1, 1, 1}, Z8[8] = {};
static const uint64_t QOFF[4] = {0, 2, 4, 6}, IDENT[4] = {0, 1, 2, 3}, ONE_GROUP[2] = {0, 3}, SEED_OFF[4] = {0, 1, 2, 3}, SEGS[3] = {0, 4, 8};
static const uint64_t CLS_GROUPS[2] = {0, 2};
static const uint32_t POS[4] = {}, CORES[4] = {0, 4, 0, 4};

static SearchRequest plain_rq()
{
    SearchRequest rq;
    rq.qbytes = B8;
    rq.qoffsets = QOFF;
    rq.nq = 3;
    return rq;
}
static SearchRequest anchored_rq()
{
    SearchRequest rq = plain_rq();
    rq.anchors = B8;
    return rq;
}
static SearchRequest terms_rq()
{
    SearchRequest rq = plain_rq();
    rq.group_offsets = ONE_GROUP;
    rq.ngroups = 1;
    rq.exclude = Z8;
    return rq;
}
static SearchRequest seq_rq()
{
    SearchRequest rq = terms_rq();
    rq.exclude = nullptr;
    rq.seq_anchors = Z8;
    return rq;
}
static SearchRequest class_rq()      // two segments, two cores, one group
{
    SearchRequest rq = seq_rq();
    rq.nq = 2;
    rq.group_offsets = CLS_GROUPS;
    rq.class_bytes = B8;
    rq.class_plane = Z8;
    rq.class_offsets = SEGS;
    rq.class_nsegs = 2;
    rq.class_groups = CLS_GROUPS;
    rq.class_cores = CORES;
    rq.class_sets = B8;
    rq.class_nsets = 1;
    rq.class_void = Z8;
    return rq;
}
static SearchRequest folded(SearchRequest rq)       // the same batch under fold: its patterns become terms, one seed query each
{
    rq.term_bytes = rq.qbytes;
    rq.term_offsets = rq.qoffsets;
    rq.nterms = rq.nq;
    rq.seed_offsets = SEED_OFF;
    rq.seed_pos = POS;
    return rq;
}
static SearchRequest near_rq()
{
    SearchRequest rq = folded(terms_rq());
    rq.group_offsets = IDENT;
    rq.ngroups = 3;
    rq.near_budget = B8;
    return rq;
}
static SearchRequest edit_rq()
{
    SearchRequest rq = near_rq();
    rq.near_edits = true;
    return rq;
}

typedef std::function<void(SearchRequest &)> Break;

static void broken(const char *what, const SearchRequest &valid, RequestVerdict want, const std::vector<Break> &clauses)
{
    CHECK(check_request(valid, 2, true) == REQUEST_OK, "%s", what);
    for (size_t k = 0; k < clauses.size(); ++k) {
        SearchRequest rq = valid;
        clauses[k](rq);
        const RequestVerdict got = check_request(rq, 2, true);
        CHECK(got == want, "%s, clause %zu: verdict %d, not %d", what, k, (int)got, (int)want);
    }
}

static void requests()
{
    static const uint64_t not_ident_a[4] = {0, 1, 1, 3}, not_ident_b[4] = {1, 1, 2, 3}, groups_short[2] = {0, 1}, groups_late[2] = {1, 2};
    // valid: plain in every mode, with low latency and the other order; ids without line tables where there is no chunk
    for (SearchMode mode : {SEARCH_FULL, SEARCH_COUNTS, SEARCH_DEVICE, SEARCH_IDS}) {
        SearchRequest rq = plain_rq();
        rq.mode = mode;
        rq.low_latency = rq.sa_order = true;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "plain, mode %d", (int)mode);
    }
    SearchRequest ids = plain_rq();
    ids.mode = SEARCH_IDS;
    CHECK(check_request(ids, 2, false) == REQUEST_IDS_WITHOUT_LINES && check_request(ids, 0, false) == REQUEST_OK, "ids");
    ids.mode = SEARCH_FULL;
    CHECK(check_request(ids, 2, false) == REQUEST_OK, "no ids, no line tables");

    broken("anchored", anchored_rq(), REQUEST_ANCHORED, {[](SearchRequest &r) { r.mode = SEARCH_DEVICE; }, [](SearchRequest &r) { r.low_latency = true; }});
    for (SearchMode mode : {SEARCH_COUNTS, SEARCH_IDS}) {
        SearchRequest rq = anchored_rq();
        rq.mode = mode;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "anchored, mode %d", (int)mode);
    }

    const std::vector<Break> group_clauses = {[](SearchRequest &r) { r.mode = SEARCH_DEVICE; }, [](SearchRequest &r) { r.low_latency = true; },
                                              [](SearchRequest &r) { r.anchors = B8; }};
    broken("all-terms", terms_rq(), REQUEST_ALL_TERMS, group_clauses);
    broken("all-terms", terms_rq(), REQUEST_ALL_TERMS, {[](SearchRequest &r) { r.exclude = nullptr; }});
    broken("sequence", seq_rq(), REQUEST_ALL_TERMS, group_clauses);
    broken("sequence", seq_rq(), REQUEST_ALL_TERMS, {[](SearchRequest &r) { r.seq_anchors = nullptr; }});
    SearchRequest none = terms_rq();        // (no term at all: nothing to flag)
    none.nq = 0;
    none.exclude = nullptr;
    CHECK(check_request(none, 2, true) == REQUEST_OK, "no terms");

    // the seeded rule: under fold (all-terms and sequence), near, edits
    const std::vector<Break> seeded_clauses = {
        [](SearchRequest &r) { r.seed_offsets = nullptr; }, [](SearchRequest &r) { r.seed_pos = nullptr; },
        [](SearchRequest &r) { r.term_bytes = nullptr; }, [](SearchRequest &r) { r.term_offsets = nullptr; },
        // (neither flags nor anchors: with queries the all-terms rule says so first, so without -- the terms stay)
        [](SearchRequest &r) { r.exclude = nullptr; r.seq_anchors = nullptr; r.nq = 0; }};
    for (const SearchRequest &valid : {folded(terms_rq()), folded(seq_rq()), near_rq(), edit_rq()}) {
        broken("seeded", valid, REQUEST_SEEDED, seeded_clauses);
        // (these three fail the all-terms rule first, which is judged first: the verdict is that rule's)
        broken("seeded", valid, REQUEST_ALL_TERMS, group_clauses);
    }
    // (the clauses the all-terms rule does not see: a seeded batch without groups)
    broken("seeded", folded(terms_rq()), REQUEST_SEEDED, {[](SearchRequest &r) { r.group_offsets = nullptr; }});
    broken("fold", folded(terms_rq()), REQUEST_SEEDED, {[](SearchRequest &r) { r.near_edits = true; }});       // near_edits without budgets
    {   // a seeded batch without terms needs neither flags nor anchors -- but the all-terms rule asks for one while there are queries
        SearchRequest rq = folded(terms_rq());
        rq.nterms = 0;
        rq.nq = 0;
        rq.exclude = nullptr;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "no terms, no flags");
    }
    for (const SearchRequest &valid : {near_rq(), edit_rq()})
        broken("budgets", valid, REQUEST_SEEDED,
               {[](SearchRequest &r) { r.seq_anchors = Z8; },                           // budgets with sequence anchors
                [](SearchRequest &r) { r.seq_anchors = Z8; r.exclude = nullptr; },
                [](SearchRequest &r) { r.ngroups = 2; },                                // not as many groups as terms
                [](SearchRequest &r) { r.nterms = 2; },
                [](SearchRequest &r) { r.group_offsets = not_ident_a; },                // groups that are not the identity
                [](SearchRequest &r) { r.group_offsets = not_ident_b; }});
    broken("near", near_rq(), REQUEST_SEEDED, {[](SearchRequest &r) { r.seed_offsets = nullptr; r.seed_pos = nullptr; }});   // budgets alone
    {
        SearchRequest rq = plain_rq();
        rq.near_edits = true;
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED, "near_edits on a plain batch");
        rq = plain_rq();
        rq.seed_pos = POS;
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED, "seed positions on a plain batch");
    }

    // the class rule, exact and under fold
    const std::vector<Break> class_clauses = {
        [](SearchRequest &r) { r.class_bytes = nullptr; }, [](SearchRequest &r) { r.class_plane = nullptr; },
        [](SearchRequest &r) { r.class_offsets = nullptr; }, [](SearchRequest &r) { r.class_groups = nullptr; },
        [](SearchRequest &r) { r.class_cores = nullptr; }, [](SearchRequest &r) { r.class_void = nullptr; },
        [](SearchRequest &r) { r.class_sets = nullptr; },                               // sets named, none stated
        [](SearchRequest &r) { r.class_nsets = 256; },
        [](SearchRequest &r) { r.class_groups = groups_short; },                        // class_groups not ending at class_nsegs
        [](SearchRequest &r) { r.class_groups = groups_late; }};                        // ... nor starting at 0
    broken("class", class_rq(), REQUEST_CLASS, class_clauses);
    broken("class under fold", folded(class_rq()), REQUEST_CLASS, class_clauses);
    {
        SearchRequest rq = class_rq();      // 255 sets are legal; no set named, none stated
        rq.class_nsets = 255;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "255 sets");
        rq.class_nsets = 0;
        rq.class_sets = nullptr;
        CHECK(check_request(rq, 2, true) == REQUEST_OK, "no sets");
        rq = class_rq();                    // more cores than segments, the groups still ending at the segments
        rq.nq = 3;
        CHECK(check_request(rq, 2, true) == REQUEST_CLASS, "three cores of two segments");
        rq = folded(class_rq());
        rq.nterms = 3;
        CHECK(check_request(rq, 2, true) == REQUEST_CLASS, "three cores of two segments, under fold");
        rq = terms_rq();                    // a class block on an all-terms batch: no sequence anchors
        rq.class_void = Z8;
        CHECK(check_request(rq, 2, true) == REQUEST_CLASS, "one member of a block on an all-terms batch");
        rq = plain_rq();                    // ... and on a plain one: no groups
        rq.class_nsegs = 1;
        CHECK(check_request(rq, 2, true) == REQUEST_CLASS, "class_nsegs on a plain batch");
        rq = plain_rq();
        rq.class_nsets = 1;
        CHECK(check_request(rq, 2, true) == REQUEST_CLASS, "class_nsets on a plain batch");
    }
    {   // budgets are another search: a near batch with a class block fails the seeded rule (sequence anchors) first
        SearchRequest rq = folded(class_rq());
        rq.near_budget = B8;
        CHECK(check_request(rq, 2, true) == REQUEST_SEEDED, "class with budgets");
    }
}

int main()
{
    layouts();
    staging();
    routes();
    requests();
    printf("search_layout: ok\n");
    return 0;
}
