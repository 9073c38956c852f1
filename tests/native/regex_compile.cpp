// tests/native/regex_compile.cpp -- csrc/regex_compile.h and the RegexBlock of csrc/search_layout.h on the CPU, built with
// g++ under AddressSanitizer + UBSan against those headers alone: no library, no device
// (tests/test_regex_host.py::test_compiler_under_sanitizers).
//
// argv[1] names a file of lines "<flags> <accept|refuse> <hex of the pattern> [<hex of a string> <0|1>]...": every pattern is
// compiled; one to refuse must be refused with a message that names a position or says "too complex"; one to accept must
// compile to a table that keeps the numbering contract, and regex_match must give the stated answer for every string.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "regex_compile.h"
#include "search_layout.h"

using namespace pss;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

static std::string unhex(const std::string &h)
{
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

// The numbering contract of a compiled pattern, and every table entry and class inside its bounds.
static void contract(const RegexDfa &d, const std::string &pat)
{
    const char *p = pat.c_str();
    CHECK(d.nstates >= 2 && d.nstates <= REGEX_MAX_STATES && d.ncls >= 1 && d.ncls <= 256, "%s: %u states, %u classes", p, d.nstates, d.ncls);
    CHECK(d.table.size() == (size_t)d.nstates * d.ncls, "%s: table size", p);
    CHECK(d.start >= 1 && d.start < d.nstates && d.first_accept >= 1 && d.first_accept <= d.nstates, "%s: start / first_accept", p);
    for (uint32_t b = 0; b < 256; ++b) CHECK(d.cls[b] < d.ncls, "%s: class of byte %u", p, b);
    for (uint16_t to : d.table) CHECK(to < d.nstates, "%s: an entry past the states", p);
    for (uint32_t c = 0; c < d.ncls; ++c) CHECK(d.table[c] == 0, "%s: the dead state leaves", p);
    if (d.anchors & REGEX_ANCHOR_END)
        CHECK(d.sink == 0, "%s: a sink under $", p);
    else {
        CHECK(d.sink == d.nstates - 1 && d.first_accept == d.sink, "%s: the sink is the one accepting state", p);
        for (uint32_t c = 0; c < d.ncls; ++c) CHECK(d.table[(size_t)d.sink * d.ncls + c] == d.sink, "%s: the sink leaves", p);
    }
    CHECK(!d.literals.empty() && d.literals.size() <= REGEX_MAX_LITERALS, "%s: %zu literals", p, d.literals.size());
    for (size_t i = 0; i + 1 < d.literals.size(); ++i) CHECK(d.literals[i].size() >= d.literals[i + 1].size(), "%s: literal order", p);
}

static void regex_block()
{
    // the regions restated: 32 bytes of header and 256 of class map per row, two bytes per table word, each rounded to 64
    struct Row { uint32_t nrow; uint64_t words; size_t hdr, cls, tables, end; };
    const Row rows[] = {{1, 1, 0, 64, 320, 384},      {1, 33, 0, 64, 320, 448},         {3, 100, 0, 128, 896, 1152},
                        {63, 0, 0, 2048, 18176, 18176}, {64, 31, 0, 2048, 18432, 18496}, {65, 32, 0, 2112, 18752, 18816}};
    for (const Row &r : rows) {
        const RegexBlock B(true, r.nrow, r.words);
        CHECK(B.hdr == r.hdr && B.cls == r.cls && B.tables == r.tables && B.end == r.end, "RegexBlock %u %llu: %zu %zu %zu %zu", r.nrow,
              (unsigned long long)r.words, B.hdr, B.cls, B.tables, B.end);
    }
    const RegexBlock none(false, 65, 1000);
    CHECK(none.end == 0 && none.tables == 0, "RegexBlock of no regex batch");
    // embedded: nothing moves in a batch without one, and the block sits between the class block and the drivers
    const ClassBlock C;
    const TermsLayout plain(65, 64, 65, C), with(65, 64, 65, C, RegexBlock(true, 65, 32));
    CHECK(plain.gdrv == plain.regex && plain.end == TermsLayout(65, 64, 65, C, RegexBlock()).end, "TermsLayout without a regex block");
    CHECK(with.regex == plain.regex && with.gdrv == with.regex + 18816 && with.end == plain.end + 18816, "TermsLayout with a regex block");
    const SeedLayout splain(64, 64, 65, 33, 64, 64, false, C), swith(64, 64, 65, 33, 64, 64, false, C, RegexBlock(true, 64, 31));
    CHECK(swith.fbytes == splain.fbytes + 18496 && swith.end == splain.end + 18496 && swith.regex == splain.regex, "SeedLayout with a regex block");
    // the request rule: a valid block passes, every broken clause is refused
    uint64_t goff[2] = {0, 1}, qoff[2] = {0, 2};
    uint8_t excl[1] = {0}, cls[256] = {}, q[2] = {'a', 'b'};
    uint16_t tab[4] = {0, 0, 1, 1};
    uint32_t hdr[REGEX_HDR_WORDS] = {0, 2, 2, 1, 1, 1, 0, 0};
    SearchRequest rq{q, qoff, 1, SEARCH_IDS, nullptr, goff, 1, excl};
    rq.regex_hdr = hdr; rq.regex_cls = cls; rq.regex_tables = tab; rq.regex_table_words = 4;
    CHECK(check_request(rq, 1, true) == REQUEST_OK, "a valid regex request");
    CHECK(BatchShape(rq, 1, 2, false, false, false).regex, "BatchShape::regex");
    { SearchRequest b = rq; b.regex_cls = nullptr; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "no class maps"); }
    { SearchRequest b = rq; b.regex_table_words = 3; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "a table past the tables"); }
    { SearchRequest b = rq; b.mode = SEARCH_DEVICE; CHECK(check_request(b, 1, true) != REQUEST_OK, "SEARCH_DEVICE"); }
    { SearchRequest b = rq; uint8_t one[1] = {1}; b.exclude = one; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "an exclude term"); }
    { SearchRequest b = rq; uint8_t a[1] = {0}; b.seq_anchors = a; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "sequence anchors"); }
    { SearchRequest b = rq; uint32_t h[REGEX_HDR_WORDS] = {0, 2, 2, 2, 1, 1, 0, 0}; b.regex_hdr = h; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "start past the states"); }
    { SearchRequest b = rq; uint32_t h[REGEX_HDR_WORDS] = {0, 4097, 1, 1, 1, 1, 0, 0}; b.regex_hdr = h; b.regex_table_words = 5000; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "too many states"); }
    { SearchRequest b = rq; uint8_t c2[256] = {}; c2[255] = 2; b.regex_cls = c2; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "a class past ncls"); }
    { SearchRequest b = rq; uint16_t t2[4] = {0, 0, 1, 2}; b.regex_tables = t2; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "an entry past the states"); }
    { SearchRequest b; b.regex_table_words = 1; CHECK(check_request(b, 1, true) == REQUEST_REGEX, "a block without a batch"); }
}

int main(int argc, char **argv)
{
    regex_block();
    if (argc < 2) {
        fprintf(stderr, "usage: regex_compile <cases>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    size_t patterns = 0, strings = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        uint32_t flags;
        std::string verdict, hex;
        if (!(ss >> flags >> verdict >> hex)) continue;
        const std::string pat = unhex(hex);
        RegexDfa d;
        std::string why;
        const bool ok = regex_compile(reinterpret_cast<const uint8_t *>(pat.data()), pat.size(), flags, &d, &why);
        ++patterns;
        if (verdict == "refuse") {
            CHECK(!ok, "%s: compiled", pat.c_str());
            CHECK(ok || why.find("position") != std::string::npos || why.find("too complex") != std::string::npos, "%s: %s", pat.c_str(), why.c_str());
            continue;
        }
        CHECK(ok, "%s: %s", pat.c_str(), why.c_str());
        if (!ok) continue;
        contract(d, pat);
        std::string shex;
        int want;
        while (ss >> shex >> want) {
            const std::string s = unhex(shex);
            const bool got = regex_match(d, reinterpret_cast<const uint8_t *>(s.data()), s.size());
            CHECK(got == (want != 0), "%s on %s: %d, not %d", pat.c_str(), shex.c_str(), (int)got, want);
            ++strings;
        }
    }
    if (failures) {
        fprintf(stderr, "regex_compile: %d failures\n", failures);
        return 1;
    }
    printf("regex_compile: ok (%zu patterns, %zu strings)\n", patterns, strings);
    return 0;
}
