// The rules of the builder's plan memory (csrc/build_plan.h) walked on the CPU.  build() below is the skeleton of one
// pss_sa_build_device call as sa_build.hip makes it -- the same calls into BuildPlan in the same order, the attempts and
// their restarts -- with the device work replaced by what a text is known to do: whether the MSD sort's bucket check
// takes it, whether its symbol counts look like log lines, whether a kept sample of another text cuts it into tiles.
// It replays the sequences of tests/test_sa_gpu.py::test_initial_sort_plan_is_reused_and_checked and
// ::test_sample_sort_plan_is_reused_across_chunks with the values those assert, and adds what they cannot afford at
// 2^24 .. 2^25 bytes a build: the whole back-off row, every argument of the hint, what a cold build forgets.
// Exit code 0 = every check holds.  Built by tests/test_host.py with g++ -fsanitize=address,undefined against build_plan.h alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "build_plan.h"

using namespace pss;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

enum : uint32_t { NO_PLAN = 2, NO_FIRST_CHUNK_SHORTCUT = 4, COLD = 8 };      // include/pss.h, PSS_SA_*

struct Text {
    uint32_t logn;
    uint32_t present[8];        // byte values that occur
    bool aligned;               // the text pointer is 16-byte aligned
    bool loglike;               // symbol counts close to uniform, no copies: a first chunk goes to the MSD sort on them alone
    bool msd_ok;                // no crowded bucket: the MSD sort (and the sizing sample's screen before it) takes the text
    int family;                 // a kept sample cuts texts of its own family into tiles, and no others
    uint64_t tag;               // geometry of the sample sort
    uint32_t radix;
};

struct Switches {
    bool plain = true;          // every knob at its default (PSS_NO_PLAN_CACHE=1: false)
    bool no_front = false;      // PSS_NO_PLAN_FRONT=1
};

struct Device {
    BuildPlan plan;
    int sample_family = 0;      // whose sorted sample lies in the slot of the kept sample (0: the slot is empty)
};

struct Report {
    int plan_hint, msd, ss, ss_planned, ss_plan_refused, restarts;
    bool tried_sample;          // some attempt cut the text with the kept sample
};

static bool subset(const uint32_t a[8], const uint32_t b[8])
{
    for (int i = 0; i < 8; ++i)
        if (a[i] & ~b[i]) return false;
    return true;
}

static Report build(Device &d, const Text &t, uint32_t flags = 0, Switches sw = Switches())
{
    BuildPlan &plan = d.plan;
    if (flags & COLD) {
        plan.forget();
        flags &= ~COLD;
    }
    Report r = {};
    for (;;) {                                  // one attempt
        const bool plain = sw.plain && (flags & NO_PLAN) == 0;
        const bool fronted = plan.fronted(t.logn, t.aligned, plain, sw.no_front);
        const bool shortcut_ok = plain && !sw.no_front && (flags & NO_FIRST_CHUNK_SHORTCUT) == 0 && t.logn >= kPlanMinLogN;
        const bool fresh = !fronted && shortcut_ok && t.aligned && t.loglike;
        const bool front_any = fronted || fresh;
        uint32_t present[8];
        uint8_t lut[256] = {};
        memcpy(present, fronted ? plan.present : t.present, 32);
        const int hint = front_any ? 1 : plan.hint(t.logn, present, plain);
        r.plan_hint = fronted ? 2 : (fresh ? 3 : hint);
        r.msd = r.ss = r.ss_planned = 0;
        if (hint == 1 || (hint == 0 && t.msd_ok)) {                 // the MSD sort is tried
            const bool accepted = t.msd_ok && (!fronted || subset(t.present, plan.present));       // (fronted: every byte needs a code)
            if (front_any && !accepted) {
                plan.refuse();
                if (fresh) flags |= NO_FIRST_CHUNK_SHORTCUT;
                ++r.restarts;
                continue;
            }
            r.msd = accepted;
        }
        if (!r.msd) {                                               // the sample sort (it takes any text with a sample of its own)
            const bool planned = plan.ss_usable(hint, t.tag, t.radix) && d.sample_family != 0;
            const bool keep = !planned && plain;
            plan.ss_begin();
            if (planned) r.tried_sample = true;
            if (planned && d.sample_family != t.family) {
                plan.ss_refused();
                r.ss_plan_refused = 1;
                ++r.restarts;
                continue;
            }
            if (keep) d.sample_family = t.family;
            plan.ss_accepted(planned, hint, planned || keep, t.tag, t.radix);
            r.ss = 1;
            r.ss_planned = planned;
        }
        if (!fronted) plan.remember_sort(t.logn, plain, present, lut, 38, r.msd != 0, r.ss != 0);
        return r;
    }
}

static Text make(uint32_t logn, const char *alphabet, bool loglike, bool msd_ok, int family, uint64_t tag)
{
    Text t = {};
    t.logn = logn;
    for (const char *c = alphabet; *c; ++c) t.present[(unsigned char)*c >> 5] |= 1u << (*c & 31);
    t.aligned = true;
    t.loglike = loglike;
    t.msd_ok = msd_ok;
    t.family = family;
    t.tag = tag;
    t.radix = 0;
    for (int i = 0; i < 8; ++i) t.radix += (uint32_t)__builtin_popcount(t.present[i]);
    t.radix += 1;
    return t;
}

static const char *kLines = "abcdefghijklmnopqrstuvwxyz0123456789 .\n";

// test_initial_sort_plan_is_reused_and_checked
static void initial_sort_plan(bool front)
{
    Switches sw;
    sw.no_front = !front;
    Device d;
    const Text lines = make(24, kLines, true, true, 1, 0x1001);
    Report r = build(d, lines, COLD, sw);
    CHECK(r.plan_hint == (front ? 3 : 0) && r.msd == 1);
    r = build(d, lines, 0, sw);
    CHECK(r.plan_hint == (front ? 2 : 1) && r.msd == 1 && r.restarts == 0);
    if (front) {
        Text shifted = lines;                   // an unaligned text pointer keeps the separate passes
        shifted.aligned = false;
        r = build(d, shifted, 0, sw);
        CHECK(r.plan_hint == 1 && r.msd == 1);
        // a byte the remembered alphabet does not have: refused inside the first pass, rebuilt as a first chunk
        const Text odd = make(24, "abcdefghijklmnopqrstuvwxyz0123456789 .\n~", true, true, 1, 0x1001);
        r = build(d, odd, 0, sw);
        CHECK(r.plan_hint == 3 && r.msd == 1 && r.restarts == 1);
        // ... which is the plan now; the old text is over a subset of that alphabet and takes the larger table
        r = build(d, lines, 0, sw);
        CHECK(r.plan_hint == 2 && r.msd == 1 && r.restarts == 0);
        CHECK(memcmp(d.plan.present, odd.present, 32) == 0);
    }
    // same alphabet, crowded prefixes
    const Text crowded = make(24, kLines, false, false, 2, 0x1001);
    r = build(d, crowded, 0, sw);
    if (front) CHECK(r.plan_hint == 0 && r.msd == 0 && r.ss == 1 && r.restarts == 1);          // planned, refused, rebuilt
    else CHECK(r.plan_hint == 1 && r.msd == 0 && r.ss == 1 && r.restarts == 0);                // hinted, refused
    r = build(d, lines, 0, sw);
    CHECK(r.plan_hint == (front ? 3 : 0) && r.msd == 1);                                      // the refusal cleared the plan
    // (without the front the crowded text's sample sort is the plan: its kept sample does not cut `lines`, and the
    // build starts over once more)
    CHECK(r.ss_plan_refused == (front ? 0 : 1) && r.restarts == (front ? 0 : 1));
    build(d, lines, 0, sw);
    Switches off = sw;
    off.plain = false;                          // PSS_NO_PLAN_CACHE=1
    r = build(d, lines, 0, off);
    CHECK(r.plan_hint == 0 && r.msd == 1);
}

// test_sample_sort_plan_is_reused_across_chunks
static void sample_sort_plan()
{
    Device d;
    const char *letters = "abcdefghijklmnopqrstuvwxyz \n";
    const Text a = make(24, letters, false, false, 1, 0x2001), b = a;
    Report r = build(d, a, COLD);
    CHECK(r.plan_hint == 0 && r.ss == 1 && r.ss_planned == 0);
    for (const Text *t : {&b, &a}) {
        r = build(d, *t);
        CHECK(r.plan_hint == 2 && r.ss == 1 && r.ss_planned == 1 && r.msd == 0);
    }
    r = build(d, b, COLD);                      // a cold build forgets, and leaves a new plan
    CHECK(r.plan_hint == 0 && r.ss_planned == 0);
    r = build(d, a);                            // (a chunk a few entries shorter: the same geometry)
    CHECK(r.ss == 1 && r.ss_planned == 1 && r.ss_plan_refused == 0);
    const Text longer = make(25, letters, false, false, 1, 0x2002);      // another size class: own sample
    r = build(d, longer);
    CHECK(r.ss == 1 && r.ss_planned == 0);
    // equal keys where no remembered splitter separates them: refused, the build starts over with a sample of its own;
    // the next chunk does not try the plan at once, the one after does
    build(d, a, COLD);
    const Text odd = make(24, letters, false, false, 2, 0x2001);
    r = build(d, odd);
    CHECK(r.ss == 1 && r.ss_planned == 0 && r.ss_plan_refused == 1 && r.restarts == 1);
    r = build(d, b);
    CHECK(r.plan_hint == 2 && r.ss_planned == 0 && r.ss_plan_refused == 0 && !r.tried_sample);
    r = build(d, a);
    CHECK(r.ss_planned == 1 && r.ss_plan_refused == 0);
    Switches off;
    off.plain = false;
    build(d, a, 0, off);
    r = build(d, b, 0, off);
    CHECK(r.plan_hint == 0 && r.ss == 1 && r.ss_planned == 0);
}

// After a refusal with back-off k exactly k builds go by without the kept sample, the next one tries it; refusal after
// refusal the row runs 1, 3, 7, 15, 31, 63, 63; a build the kept sample cuts starts the row again.
static void back_off()
{
    Device d;
    const char *letters = "abcdefghijklmnopqrstuvwxyz \n";
    const Text a = make(24, letters, false, false, 1, 0x2001);
    Text other = a;
    build(d, a, COLD);
    const uint32_t row[] = {1, 3, 7, 15, 31, 63, 63};
    int family = 2;
    for (uint32_t k : row) {
        other.family = ++family;                // (no kept sample ever cuts the next text)
        Report r = build(d, other);
        CHECK(r.tried_sample && r.ss_plan_refused == 1 && r.ss_planned == 0 && r.restarts == 1);
        CHECK(d.plan.ss_backoff == k && d.plan.ss_skip == k);
        for (uint32_t i = 0; i < k; ++i) {
            r = build(d, other);
            CHECK(r.plan_hint == 2 && !r.tried_sample && r.ss == 1 && r.ss_planned == 0 && r.restarts == 0);
            CHECK(d.plan.ss_skip == k - 1 - i && d.plan.ss_backoff == k);
        }
    }
    Report r = build(d, other);                 // the sample the last of them kept
    CHECK(r.tried_sample && r.ss_planned == 1 && d.plan.ss_backoff == 0 && d.plan.ss_skip == 0);
    other.family = ++family;
    r = build(d, other);
    CHECK(r.ss_plan_refused == 1 && d.plan.ss_backoff == 1);
}

static void hint_arguments()
{
    Device d;
    const Text lines = make(24, kLines, true, true, 1, 0x1001);
    build(d, lines, COLD);
    const BuildPlan &p = d.plan;
    CHECK(p.path == 1 && p.logn == 24);
    CHECK(p.fronted(24, true, true, false));
    CHECK(!p.fronted(25, true, true, false));           // another size class
    CHECK(!p.fronted(24, false, true, false));          // an unaligned pointer
    CHECK(!p.fronted(24, true, false, false));          // a switch off its default
    CHECK(!p.fronted(24, true, true, true));            // PSS_NO_PLAN_FRONT
    CHECK(p.hint(24, lines.present, true) == 1);
    CHECK(p.hint(25, lines.present, true) == 0);
    CHECK(p.hint(24, lines.present, false) == 0);
    uint32_t more[8];
    memcpy(more, lines.present, 32);
    more['~' >> 5] |= 1u << ('~' & 31);
    CHECK(p.hint(24, more, true) == 0);                 // another set of byte values
    // below the size class nothing is remembered and nothing is used
    Device small;
    Text tiny = lines;
    tiny.logn = 23;
    Report r = build(small, tiny, COLD);
    CHECK(r.plan_hint == 0 && small.plan.path == 0 && small.plan.logn == 0);
    BuildPlan forced = p;
    forced.logn = 23;
    CHECK(!forced.fronted(23, true, true, false) && forced.hint(23, lines.present, true) == 0);
    // the sample sort's path is never fronted, and its hint is 2
    BuildPlan q = p;
    q.path = 2;
    CHECK(!q.fronted(24, true, true, false) && q.hint(24, lines.present, true) == 2);
    // the kept sample: hint 2, the same geometry and radix, no builds left to go by
    q.ss_tag = 7;
    q.ss_radix = 39;
    CHECK(q.ss_usable(2, 7, 39) && !q.ss_usable(1, 7, 39) && !q.ss_usable(2, 8, 39) && !q.ss_usable(2, 7, 40) && !q.ss_usable(2, 0, 39));
    q.ss_skip = 1;
    CHECK(!q.ss_usable(2, 7, 39));
    // the side line's depth: same size class, same bits per symbol, plain
    q.remember_side(24, 6, true, 22);
    CHECK(q.side_depth(24, 6, true) == 22 && q.side_depth(25, 6, true) == 0 && q.side_depth(24, 5, true) == 0 && q.side_depth(24, 6, false) == 0);
    q.remember_side(23, 6, true, 30);                   // (below the size class: not written)
    q.remember_side(24, 6, false, 30);
    CHECK(q.side_depth(24, 6, true) == 22);
    q.remember_side(24, 6, true, 0);
    CHECK(q.side_depth(24, 6, true) == 0);
}

// A cold build clears the remembered path, the back-off and its countdown, and the side line's depth -- nothing else.
static void forget_clears_four()
{
    BuildPlan p;
    memset(p.present, 0x5a, sizeof p.present);
    memset(p.lut, 0x17, sizeof p.lut);
    p.logn = 24; p.path = 2; p.sigma = 38;
    p.ss_tag = 0x2001; p.ss_radix = 39; p.ss_skip = 3; p.ss_backoff = 7;
    p.side_heff = 22; p.side_logn = 24; p.side_b = 6;
    BuildPlan want = p;
    want.path = 0;
    want.ss_skip = want.ss_backoff = 0;
    want.side_heff = 0;
    p.forget();
    CHECK(memcmp(p.present, want.present, 32) == 0 && memcmp(p.lut, want.lut, 256) == 0);
    CHECK(p.logn == want.logn && p.path == want.path && p.sigma == want.sigma);
    CHECK(p.ss_tag == want.ss_tag && p.ss_radix == want.ss_radix && p.ss_skip == want.ss_skip && p.ss_backoff == want.ss_backoff);
    CHECK(p.side_heff == want.side_heff && p.side_logn == want.side_logn && p.side_b == want.side_b);
    BuildPlan q = want;
    q.path = 1; q.ss_skip = 3; q.ss_backoff = 7; q.side_heff = 22;
    q.refuse();                                 // ... and a refusal the path alone
    CHECK(q.path == 0 && q.ss_skip == 3 && q.ss_backoff == 7 && q.side_heff == 22 && q.ss_tag == want.ss_tag && q.logn == want.logn);
}

int main()
{
    initial_sort_plan(true);
    initial_sort_plan(false);
    sample_sort_plan();
    back_off();
    hint_arguments();
    forget_clears_four();
    puts("build_plan: ok");
    return 0;
}
