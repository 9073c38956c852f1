// span_core.cpp -- the scoring and key functions of the match spans (csrc/span_core.h) on the CPU, start
// by start as the 64 lanes of span_kernel (csrc/span_impl.h) run them: recorded cases in, every answer compared with the
// recorded one.  Header only: no library, no device.  (tests/test_span_host.py writes the cases with the brute-force
// reference of tests/span_ref.py and builds this with g++ under AddressSanitizer + UBSan.)
//
// Every text lies FLUSH with the start of a heap block of exactly n + 128 bytes -- the zero padding a reader guarantees
// behind a chunk's n bytes -- and every pattern in a block of exactly L + kSpanPatPad bytes, so a read below offset 0, past
// the padding, or past the pattern's padding is a sanitizer report; a read that takes the padding for text is a wrong answer.
//
// Case file: u32 count, then per case u32 n, n bytes of chunk text, u32 line, u32 L, L pattern bytes, u8 k, u8 flags
// (1 = edits, 2 = icase), 3 x i32 the expected start, length, distance.  Little endian, no alignment.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "span_core.h"

using namespace pss;

constexpr uint32_t kTextPad = 128;      // (search.h, ChunkDesc: readable 128 bytes past the end, zero filled)
constexpr uint32_t kLanes = 64;

struct In {
    const uint8_t *p, *end;
    bool ok = true;
    void take(void *out, size_t len)
    {
        if ((size_t)(end - p) < len) {
            ok = false;
            memset(out, 0, len);
            return;
        }
        memcpy(out, p, len);
        p += len;
    }
    uint32_t u32() { uint32_t v; take(&v, 4); return v; }
    uint8_t u8() { uint8_t v; take(&v, 1); return v; }
};

// One row as the kernel walks it: steps of 64 starts, the least key of a step, the least over the steps, out after a step
// that found distance 0.
template <bool kFold, bool kEdits>
static uint64_t walk(const uint8_t *text, uint32_t n, uint32_t es, uint32_t elen, const uint8_t *pat, uint32_t L, uint32_t k)
{
    const uint32_t starts = span_starts(elen, L, kEdits);
    uint64_t best = kSpanNone;
    for (uint32_t base = 0; base < starts; base += kLanes) {
        uint64_t step = kSpanNone;
        for (uint32_t lane = 0; lane < kLanes; ++lane) {
            const uint32_t s = base + lane;
            const uint64_t key = s < starts ? span_start_key<kFold, kEdits>(text, n, es, elen, s, pat, L, k) : kSpanNone;
            step = key < step ? key : step;
        }
        best = step < best ? step : best;
        if ((best >> 35) == 0) break;
    }
    return best;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::printf("usage: span_core CASES\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::printf("span_core: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + got);
    std::fclose(f);
    In in{file.data(), file.data() + file.size()};
    const uint32_t count = in.u32();
    uint32_t failures = 0, matched = 0, late = 0;
    for (uint32_t c = 0; c < count && in.ok; ++c) {
        const uint32_t n = in.u32();
        if (!in.ok || n > (1u << 20)) break;
        uint8_t *text = static_cast<uint8_t *>(std::malloc((size_t)n + kTextPad));
        in.take(text, n);
        memset(text + n, 0, kTextPad);
        const uint32_t line = in.u32(), L = in.u32();
        if (!in.ok || L > (1u << 20)) {
            std::free(text);
            break;
        }
        uint8_t *pat = static_cast<uint8_t *>(std::malloc((size_t)L + kSpanPatPad));
        in.take(pat, L);
        memset(pat + L, 0, kSpanPatPad);
        const uint32_t k = in.u8(), flags = in.u8();
        int32_t want[3], got[3];
        in.take(want, sizeof want);
        if (in.ok) {
            // the entry of the row: behind `line` newlines, up to the next one or to n
            uint32_t es = 0, seen = 0;
            while (seen < line && es < n) seen += text[es++] == '\n' ? 1u : 0u;
            uint32_t end = es;
            while (end < n && text[end] != '\n') ++end;
            const bool edits = flags & 1, icase = flags & 2;
            const bool has_nl = memchr(pat, '\n', L) != nullptr;
            if (icase)
                for (uint32_t i = 0; i < L; ++i) pat[i] = (uint8_t)((uint8_t)(pat[i] - 'A') < 26 ? pat[i] | 0x20 : pat[i]);
            uint64_t key = kSpanNone;
            if (seen == line && es < n && !has_nl && k <= kSpanMaxBudget && L > k) {
                const uint32_t elen = end - es;
                key = icase ? (edits ? walk<true, true>(text, n, es, elen, pat, L, k) : walk<true, false>(text, n, es, elen, pat, L, k))
                            : (edits ? walk<false, true>(text, n, es, elen, pat, L, k) : walk<false, false>(text, n, es, elen, pat, L, k));
            }
            span_unkey(key, L, got);
            matched += got[2] >= 0 ? 1u : 0u;
            late += got[0] >= (int32_t)kLanes ? 1u : 0u;
            if (memcmp(got, want, sizeof got) != 0) {
                if (++failures <= 10)
                    std::printf("FAILED case %u (n = %u, line %u, L = %u, k = %u, flags %u): (%d, %d, %d), expected (%d, %d, %d)\n", c, n, line,
                                L, k, flags, got[0], got[1], got[2], want[0], want[1], want[2]);
            }
        }
        std::free(pat);
        std::free(text);
    }
    if (!in.ok || in.p != in.end) {
        std::printf("span_core: the case file is malformed\n");
        return 2;
    }
    if (failures) {
        std::printf("span_core: %u of %u case(s) FAILED\n", failures, count);
        return 1;
    }
    std::printf("span_core: ok, %u cases, %u with a match, %u of them behind the first step\n", count, matched, late);
    return 0;
}
