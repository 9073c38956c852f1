// build_plan.h -- what a build leaves for the next build on its device (DeviceCtx::plan), and the rules that read and
// write it.  Plain C++ without HIP: the rules are pure functions of their arguments and the struct's fields
// (tests/native/build_plan.cpp walks them on the CPU); sa_build.hip is their only caller.
#pragma once
#include <cstdint>
#include <cstring>

namespace pss {

// The size class from which builds remember: texts of at least 2^24 bytes (logn = floor(log2 n)).
constexpr uint32_t kPlanMinLogN = 24;
constexpr uint32_t kPlanMinN = 1u << kPlanMinLogN;

struct BuildPlan {
    // Which initial sort the last build on this device took, and for what kind of text (the byte values present, the
    // size class): consecutive chunks of one corpus take the same one, so the next build skips the sizing sample that
    // would only say so again (sa_build.hip; a wrong guess is caught by the sorts' own exact checks and costs one restart).
    uint32_t present[8] = {};
    uint32_t logn = 0;
    int path = 0;                        // 0 none, 1 hybrid MSD, 2 sample sort
    uint8_t lut[256] = {};               // ... and its byte -> code table (the next build recodes with it inside the sort)
    uint32_t sigma = 0;
    // ... 2: it took the sample sort, whose sorted sample (slot S_SSPLAN of sa_build.hip) cuts the next chunk of that
    // exact size and alphabet too
    uint64_t ss_tag = 0;                 // ss_geometry_tag() of the text the sample came from (0: none)
    uint32_t ss_radix = 0;
    uint32_t ss_skip = 0, ss_backoff = 0;                // builds that go by before the plan is tried again after a refusal
    // ... and whether its anchors were sorted beside the text round (sa_build.hip, SideAnchors): the depth that side line
    // was started for, the size class and the bits per symbol.  The next chunk of that kind starts its side line at once --
    // beside the initial sort as well -- instead of waiting for a sample of its ties to show copies.
    uint64_t side_heff = 0;
    uint32_t side_logn = 0;
    int side_b = 0;

    // `plain`: every switch of the builder is at its default and the caller did not ask for a build without shortcuts.
    static bool remembers(uint32_t logn_, bool plain) { return plain && logn_ >= kPlanMinLogN; }

    // A cold build: nothing of earlier builds on this device is used.
    void forget()
    {
        path = 0;
        ss_skip = ss_backoff = 0;
        side_heff = 0;
    }
    // The remembered sort did not take this text.
    void refuse() { path = 0; }

    // The last build took the MSD sort on a text of this size class: this one does not look at its alphabet first
    // either, it recodes with `lut` inside the sort's first pass (which reads the raw text in 16-byte vectors).
    bool fronted(uint32_t logn_, bool aligned16, bool plain, bool no_front) const
    {
        return remembers(logn_, plain) && !no_front && path == 1 && logn == logn_ && aligned16;
    }
    // The alphabet is known: 1 / 2 = go straight to that sort without a sizing sample, 0 = no plan for this kind of text.
    int hint(uint32_t logn_, const uint32_t present_[8], bool plain) const
    {
        return remembers(logn_, plain) && path && logn == logn_ && memcmp(present, present_, 32) == 0 ? path : 0;
    }
    // (the MSD sort's own exact check can refuse a text; the sample sort takes any text, and a bucket beyond a tile --
    // with remembered splitters as unlikely as with fresh ones -- declines: both start over without the plan)
    void remember_sort(uint32_t logn_, bool plain, const uint32_t present_[8], const uint8_t lut_[256], uint32_t sigma_, bool msd, bool ss)
    {
        if (!remembers(logn_, plain)) return;
        path = msd ? 1 : (ss && ss_tag != 0 ? 2 : 0);
        logn = logn_;
        memcpy(present, present_, 32);
        memcpy(lut, lut_, 256);
        sigma = sigma_;
    }

    // The sample sort.  May the kept sample cut a text of this geometry (the same sample size, bucket counts, index bits
    // and symbols per key: chunks of one Writer differ by an entry or two)?
    bool ss_usable(int hint_, uint64_t tag, uint32_t radix) const
    {
        return hint_ == 2 && tag != 0 && ss_tag == tag && ss_radix == radix && ss_skip == 0;
    }
    void ss_begin() { ss_tag = 0; }      // (valid again once this sort has been accepted)
    // The kept sample left a bucket beyond a tile.  The build starts over without the plan, and the next chunks do not
    // try it again at once: 1, 3, 7, ... builds go by first.
    void ss_refused()
    {
        ss_backoff = 2 * ss_backoff + 1 < 63u ? 2 * ss_backoff + 1 : 63u;
        ss_skip = ss_backoff;
        path = 0;                        // all over again without the plan: this may not be natural text at all
    }
    // sample: one was used or kept, and it lies in S_SSPLAN
    void ss_accepted(bool planned, int hint_, bool sample, uint64_t tag, uint32_t radix)
    {
        if (planned) ss_backoff = 0;
        else if (hint_ == 2 && ss_skip) --ss_skip;       // (a chunk that went by without trying)
        if (sample) {
            ss_tag = tag;
            ss_radix = radix;
        }
    }

    // The depth the last build's side line was started for, if this text is of its kind (else 0).
    uint64_t side_depth(uint32_t logn_, int b, bool plain) const
    {
        return remembers(logn_, plain) && side_logn == logn_ && side_b == b ? side_heff : 0;
    }
    void remember_side(uint32_t logn_, int b, bool plain, uint64_t heff)     // heff 0: the anchors were not sorted on the side
    {
        if (!remembers(logn_, plain)) return;
        side_heff = heff;
        side_logn = logn_;
        side_b = b;
    }
};

}  // namespace pss
