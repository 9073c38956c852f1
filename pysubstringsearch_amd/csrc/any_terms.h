// any_terms.h -- the normalisation of an any-of set (include/pss.h, pss_reader_search_any_batch): what the
// host does to a set of alternatives before the device is asked.  Plain C++ without HIP, like search_layout.h and
// regex_compile.h: tests/native/any_request.cpp builds it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace pss {

constexpr uint32_t ANY_MAX_ALTS = 64;           // PSS_ANY_MAX_ALTS: alternatives of one set after normalisation ...
constexpr uint32_t ANY_MAX_ALTS_FOLD = 32;      // ... and under fold, where every alternative needs a seed of one letter at least

// One set, normalised.  `alts` ascending bytewise (unsigned bytes, a proper prefix first) and prefix-free; none is empty.
// An empty `alts` is a set whose alternatives all held a 0x0A: it matches nothing.
struct AnySet {
    std::vector<std::string> alts;
};

inline uint8_t any_fold_byte(uint8_t b) { return (uint8_t)(b - 'A') < 26 ? (uint8_t)(b | 0x20) : b; }

// The steps, in this order:
//   1. under fold every alternative is folded to lower case (A-Z alone: `@`, `[`, 0xC9 stay what they are);
//   2. duplicates go;
//   3. an alternative that holds a 0x0A goes: it occurs in no entry.  It voids itself, not its set;
//   4. an alternative that holds another one as a substring goes: it asks nothing more of an entry than the shorter one;
//   5. the rest is sorted ascending bytewise.
// What is left is prefix-free (a prefix is a substring), so no two alternatives can start at one text position.
// The caller has refused an empty set and an empty alternative.  n alternatives cost O(n^2) substring searches: a set is
// a few dozen strings.
inline AnySet any_normalise(const uint8_t *bytes, const uint64_t *offsets, uint64_t first, uint64_t last, bool fold)
{
    std::vector<std::string> all;
    all.reserve((size_t)(last - first));
    for (uint64_t a = first; a < last; ++a) {
        std::string s(reinterpret_cast<const char *>(bytes) + offsets[a], (size_t)(offsets[a + 1] - offsets[a]));
        if (fold)
            for (char &c : s) c = (char)any_fold_byte((uint8_t)c);
        if (s.find('\n') == std::string::npos) all.push_back(std::move(s));
    }
    // (std::string compares as unsigned bytes, a proper prefix first: the order of the suffix arrays)
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    AnySet out;
    for (size_t i = 0; i < all.size(); ++i) {
        bool holds_another = false;
        for (size_t j = 0; j < all.size() && !holds_another; ++j)
            holds_another = j != i && all[j].size() < all[i].size() && all[i].find(all[j]) != std::string::npos;
        if (!holds_another) out.alts.push_back(all[i]);
    }
    return out;
}

// Letters of every alternative's seed under fold: min(letters, floor(log2(64 / n))) for a set of n <= 32 alternatives, so
// that the set -- one term of the seeded kernels -- keeps at most 64 queries.  n = 0: the configured letters (no seed is cut).
inline uint32_t any_seed_letters(uint32_t n, uint32_t letters)
{
    uint32_t f = 0;
    while (n && (64u / n) >> (f + 1)) ++f;
    return n && f < letters ? f : letters;
}

}  // namespace pss
