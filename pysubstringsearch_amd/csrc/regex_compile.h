// regex_compile.h -- a regular expression over bytes compiled to what the regex search runs on (include/pss.h,
// pss_regex_compile): the REQUIRED LITERALS that drive the search as an all-terms group, and a DFA of the
// WHOLE-ENTRY language that the verify step walks (regex_impl.h on the device, regex_match() here, the same walk).
// Plain C++ without HIP, like search_layout.h: tests/native/regex_compile.cpp builds it alone.
//
// The syntax is a subset of Python's `re` over bytes (pss.h lists it and what is refused).  parse -> a tree; Glushkov
// positions with counted repeats unrolled (position 0 is the start marker; at most REGEX_MAX_POSITIONS); byte classes;
// subset construction of `[^\n]* R [^\n]*`, the leading part dropped under `^`, the trailing one under `$`.  No
// minimization.
//
// State numbering (part of the contract): 0 is dead; the accepting states are >= first_accept; without `$` there is ONE
// accepting state, `sink`, and it absorbs every byte (an entry holds no 0x0A, so nothing can leave `[^\n]*`); with `$`
// sink is 0, "none".  The table is u16 T[nstates][ncls], a byte b read in state s leads to T[s * ncls + cls[b]].
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace pss {

constexpr uint32_t REGEX_ICASE = 1;                 // PSS_REGEX_ICASE
constexpr uint32_t REGEX_ANCHOR_START = 1, REGEX_ANCHOR_END = 2;
constexpr uint32_t REGEX_MAX_POSITIONS = 2048;      // Glushkov positions, the start marker not counted
constexpr uint32_t REGEX_MAX_STATES = 4096;         // PSS_REGEX_MAX_STATES
constexpr uint32_t REGEX_MAX_LITERALS = 8;
constexpr int REGEX_MAX_DEPTH = 200;                // groups inside groups: the parser and everything behind it recurse once per level
constexpr uint64_t REGEX_MAX_TABLE_BYTES = (uint64_t)64 << 20;      // the tables of one batch

struct RegexDfa {
    uint32_t nstates = 0, ncls = 0, start = 0, first_accept = 0, sink = 0, anchors = 0;
    uint8_t cls[256] = {};
    std::vector<uint16_t> table;                    // nstates * ncls
    std::vector<std::string> literals;              // at most REGEX_MAX_LITERALS, the longest first; folded under REGEX_ICASE
    uint64_t table_bytes() const { return (uint64_t)table.size() * 2; }
};

// The walk of regex_verify_kernel, byte by byte: stop at 0 and at sink, keep iff the last state accepts.
inline bool regex_match(const RegexDfa &d, const uint8_t *bytes, uint64_t len)
{
    uint32_t s = d.start;
    for (uint64_t i = 0; i < len && s != 0 && s != d.sink; ++i) s = d.table[(size_t)s * d.ncls + d.cls[bytes[i]]];
    return s >= d.first_accept;
}

namespace regex_detail {

struct ByteSet {
    uint64_t w[4] = {0, 0, 0, 0};
    void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
    void add_range(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; ++b) add(b); }
    bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
    void merge(const ByteSet &o) { for (int i = 0; i < 4; ++i) w[i] |= o.w[i]; }
    void negate() { for (int i = 0; i < 4; ++i) w[i] = ~w[i]; }
    bool operator==(const ByteSet &o) const { return !memcmp(w, o.w, sizeof w); }
    void fold_close()                               // both cases of every ASCII letter it holds
    {
        for (uint32_t c = 'a'; c <= 'z'; ++c)
            if (has(c) || has(c - 32)) { add(c); add(c - 32); }
    }
};

inline ByteSet class_set(char k)                    // \d \w \s and their complements, ASCII as `re` has them on bytes
{
    ByteSet s;
    switch (k | 0x20) {
    case 'd': s.add_range('0', '9'); break;
    case 'w': s.add_range('0', '9'); s.add_range('a', 'z'); s.add_range('A', 'Z'); s.add('_'); break;
    default: s.add(' '); s.add_range('\t', '\r'); break;
    }
    if (!(k & 0x20)) s.negate();
    return s;
}

enum NodeKind { N_CHAR, N_EMPTY, N_CAT, N_ALT, N_REPEAT };
constexpr uint32_t INF = 0xffffffffu;

struct Node {
    NodeKind kind = N_EMPTY;
    ByteSet set;                                    // N_CHAR
    int lit = -1;                                   // N_CHAR: the byte of a position written as ONE byte (folded under icase), else -1
    uint32_t lo = 0, hi = 0;                        // N_REPEAT
    std::vector<std::unique_ptr<Node>> kids;
};
using NodeP = std::unique_ptr<Node>;

struct Error {
    std::string msg;
};

struct Parser {
    const uint8_t *p;
    uint64_t n, i = 0;
    bool icase;
    uint32_t anchors = 0;
    int depth = 0;
    bool top_alt = false;

    [[noreturn]] void fail(uint64_t at, const char *what) const
    {
        throw Error{std::string(what) + " at position " + std::to_string(at)};
    }
    static int hexval(uint32_t c)
    {
        if (c - '0' < 10u) return (int)(c - '0');
        c |= 0x20;
        return c - 'a' < 6u ? (int)(c - 'a' + 10) : -1;
    }
    NodeP literal(uint32_t b) const
    {
        NodeP nd(new Node);
        nd->kind = N_CHAR;
        if (icase && b - 'A' < 26u) b |= 0x20;
        nd->lit = (int)b;
        nd->set.add(b);
        if (icase) nd->set.fold_close();
        return nd;
    }
    NodeP of_set(const ByteSet &s) const
    {
        NodeP nd(new Node);
        nd->kind = N_CHAR;
        nd->set = s;
        return nd;
    }
    // The escape at i (p[i] == '\\'): one byte (*byte >= 0) or a class (*byte = -1, *cls filled).  in_set: inside [...].
    void escape(bool in_set, int *byte, ByteSet *cls)
    {
        const uint64_t at = i;
        if (i + 1 >= n) fail(at, "a pattern ends in a backslash");
        const uint32_t c = p[i + 1];
        i += 2;
        *byte = -1;
        switch (c) {
        case 't': *byte = '\t'; return;
        case 'r': *byte = '\r'; return;
        case 'n': *byte = '\n'; return;
        case 'f': *byte = '\f'; return;
        case 'v': *byte = '\v'; return;
        case 'a': *byte = '\a'; return;
        case '0':
            if (i < n && (uint32_t)(p[i] - '0') < 10u) fail(at, "an octal escape (write \\xHH)");
            *byte = 0;
            return;
        case 'x': {
            const int h = i + 1 < n ? hexval(p[i]) : -1, l = i + 1 < n ? hexval(p[i + 1]) : -1;
            if (h < 0 || l < 0) fail(at, "\\x needs two hex digits");
            i += 2;
            *byte = h * 16 + l;
            return;
        }
        case 'd': case 'D': case 'w': case 'W': case 's': case 'S': *cls = class_set((char)c); return;
        case 'b': case 'B': case 'A': case 'Z': fail(at, "\\b, \\B, \\A and \\Z are not supported");
        default: break;
        }
        if (c - '1' < 9u) fail(at, "a back-reference is not supported");
        if ((c | 0x20) - 'a' < 26u) fail(at, "an unknown escape");
        if (in_set && c >= 0x80) fail(at, "a raw byte >= 0x80 inside a set (a set is one byte: write \\xHH)");
        *byte = (int)c;                              // escaped punctuation (or, outside a set, a byte >= 0x80)
    }
    NodeP set_item()
    {
        const uint64_t open = i++;                  // behind '['
        bool neg = false;
        if (i < n && p[i] == '^') { neg = true; ++i; }
        ByteSet s;
        bool first = true;
        for (;;) {
            if (i >= n) fail(open, "a set without its ]");
            if (p[i] == ']' && !first) { ++i; break; }
            first = false;
            int lo;
            ByteSet cls;
            const uint64_t at = i;
            if (p[i] == '\\')
                escape(true, &lo, &cls);
            else {
                if (p[i] >= 0x80) fail(at, "a raw byte >= 0x80 inside a set (a set is one byte: write \\xHH)");
                lo = p[i++];
            }
            if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') {      // a range lo-hi
                if (lo < 0) fail(at, "a class escape as the end of a range");
                ++i;
                int hi;
                ByteSet c2;
                if (p[i] == '\\')
                    escape(true, &hi, &c2);
                else {
                    if (p[i] >= 0x80) fail(i, "a raw byte >= 0x80 inside a set (a set is one byte: write \\xHH)");
                    hi = p[i++];
                }
                if (hi < 0) fail(at, "a class escape as the end of a range");
                if (hi < lo) fail(at, "a range that runs backwards");
                s.add_range((uint32_t)lo, (uint32_t)hi);
            } else if (lo < 0)
                s.merge(cls);
            else
                s.add((uint32_t)lo);
        }
        if (icase) s.fold_close();
        if (neg) s.negate();
        return of_set(s);
    }
    // A quantifier behind an atom, if one stands at i.
    bool quantifier(uint32_t *lo, uint32_t *hi)
    {
        if (i >= n) return false;
        const uint64_t at = i;
        const uint32_t c = p[i];
        if (c == '*') { *lo = 0; *hi = INF; ++i; }
        else if (c == '+') { *lo = 1; *hi = INF; ++i; }
        else if (c == '?') { *lo = 0; *hi = 1; ++i; }
        else if (c == '{') {
            uint64_t j = i + 1, a = 0, b = 0;
            bool have_a = false, have_b = false, comma = false;
            auto digits = [&](uint64_t *v, bool *have) {
                while (j < n && (uint32_t)(p[j] - '0') < 10u) {
                    *v = std::min<uint64_t>(*v * 10 + (p[j] - '0'), 1u << 20);
                    *have = true;
                    ++j;
                }
            };
            digits(&a, &have_a);
            if (j < n && p[j] == ',') { comma = true; ++j; digits(&b, &have_b); }
            if (j >= n || p[j] != '}' || (!have_a && !have_b)) fail(at, "a malformed {} (a literal brace is \\{)");
            *lo = (uint32_t)a;
            *hi = comma ? (have_b ? (uint32_t)b : INF) : (uint32_t)a;
            if (*hi < *lo) fail(at, "a repeat whose minimum is above its maximum");
            i = j + 1;
        } else
            return false;
        if (i < n && p[i] == '?') fail(i, "a lazy quantifier is not supported");
        if (i < n && p[i] == '+') fail(i, "a possessive quantifier is not supported");
        if (i < n && (p[i] == '*' || p[i] == '{')) fail(i, "a repeat of a repeat");
        return true;
    }
    NodeP atom()
    {
        const uint64_t at = i;
        const uint32_t c = p[i];
        if (c == '(') {
            ++i;
            if (i < n && p[i] == '?') {
                if (i + 1 < n && p[i + 1] == ':')
                    i += 2;
                else if (i + 1 < n && (p[i + 1] == '=' || p[i + 1] == '!' || p[i + 1] == '<'))
                    fail(at, "look-around is not supported");
                else if (i + 1 < n && p[i + 1] == 'P')
                    fail(at, "a named group is not supported");
                else
                    fail(at, "inline flags and (?...) extensions are not supported");
            }
            if (depth >= REGEX_MAX_DEPTH) fail(at, "groups nested more than 200 deep");
            ++depth;
            NodeP inner = alternation();
            --depth;
            if (i >= n || p[i] != ')') fail(at, "a group without its )");
            ++i;
            return inner;
        }
        if (c == '[') return set_item();
        if (c == '.') {
            ++i;
            ByteSet s;
            s.add('\n');
            s.negate();
            return of_set(s);
        }
        if (c == '\\') {
            int b;
            ByteSet cls;
            escape(false, &b, &cls);
            return b >= 0 ? literal((uint32_t)b) : of_set(cls);
        }
        if (c == '*' || c == '+' || c == '?') fail(at, "nothing to repeat");
        if (c == '{') fail(at, "a malformed {} (a literal brace is \\{)");
        if (c == '^') fail(at, "^ anywhere but at the pattern's start");
        if (c == '$') fail(at, "$ anywhere but at the pattern's end");
        ++i;
        return literal(c);
    }
    NodeP concatenation()
    {
        NodeP cat(new Node);
        cat->kind = N_CAT;
        while (i < n && p[i] != '|' && p[i] != ')') {
            if (p[i] == '^' && i == 0) { anchors |= REGEX_ANCHOR_START; ++i; continue; }
            if (p[i] == '$' && i == n - 1) { anchors |= REGEX_ANCHOR_END; ++i; continue; }
            NodeP a = atom();
            uint32_t lo, hi;
            if (quantifier(&lo, &hi)) {
                NodeP r(new Node);
                r->kind = N_REPEAT;
                r->lo = lo;
                r->hi = hi;
                r->kids.push_back(std::move(a));
                a = std::move(r);
            }
            cat->kids.push_back(std::move(a));
        }
        if (cat->kids.empty()) { cat->kind = N_EMPTY; return cat; }
        if (cat->kids.size() == 1) return std::move(cat->kids[0]);
        return cat;
    }
    NodeP alternation()
    {
        NodeP first = concatenation();
        if (i >= n || p[i] != '|') return first;
        if (depth == 0) top_alt = true;
        NodeP alt(new Node);
        alt->kind = N_ALT;
        alt->kids.push_back(std::move(first));
        while (i < n && p[i] == '|') {
            ++i;
            alt->kids.push_back(concatenation());
        }
        return alt;
    }
    NodeP parse()
    {
        if (n == 0) throw Error{"an empty pattern at position 0 (every entry matches it)"};
        NodeP root = alternation();
        if (i < n) fail(i, "a ) without its group");
        if (anchors && top_alt) throw Error{"^ or $ beside a bare alternation at position 0 (write ^(a|b))"};
        return root;
    }
};

// ---- required literals ---------------------------------------------------------------------------------------------
// Of a node: `exact`, when it matches one string and no other; else the literal run every match begins with and the one
// every match ends with; and the runs that are complete inside it.
struct Lits {
    bool is_exact = false;
    std::string exact, prefix, suffix;
    std::vector<std::string> inner;
};

inline Lits literals_of(const Node &nd)
{
    Lits out;
    switch (nd.kind) {
    case N_EMPTY: out.is_exact = true; break;
    case N_CHAR:
        if (nd.lit >= 0) { out.is_exact = true; out.exact.assign(1, (char)nd.lit); }
        break;
    case N_ALT: break;
    case N_REPEAT: {
        if (nd.lo == 0) break;
        Lits k = literals_of(*nd.kids[0]);
        if (k.is_exact && nd.lo == nd.hi && (uint64_t)k.exact.size() * nd.lo <= 256) {
            out.is_exact = true;
            for (uint32_t r = 0; r < nd.lo; ++r) out.exact += k.exact;
        } else if (k.is_exact) {
            out.prefix = out.suffix = k.exact;
            if (!k.exact.empty()) out.inner.push_back(k.exact);
        } else
            out = std::move(k);
        break;
    }
    case N_CAT: {
        bool all_exact = true;
        std::string run;
        for (const auto &kid : nd.kids) {
            Lits k = literals_of(*kid);
            if (k.is_exact) { run += k.exact; continue; }
            run += k.prefix;
            if (all_exact) out.prefix = run;
            if (!run.empty()) out.inner.push_back(run);
            for (auto &s : k.inner) out.inner.push_back(std::move(s));
            run = k.suffix;
            all_exact = false;
        }
        if (all_exact) { out.is_exact = true; out.exact = run; }
        else {
            out.suffix = run;
            if (!run.empty()) out.inner.push_back(run);
        }
        break;
    }
    }
    return out;
}

inline std::vector<std::string> required_literals(const Node &root)
{
    Lits k = literals_of(root);
    std::vector<std::string> all;
    if (k.is_exact) { if (!k.exact.empty()) all.push_back(k.exact); }
    else all = std::move(k.inner);
    std::vector<std::string> distinct;
    for (auto &s : all)
        if (std::find(distinct.begin(), distinct.end(), s) == distinct.end()) distinct.push_back(s);
    std::stable_sort(distinct.begin(), distinct.end(), [](const std::string &a, const std::string &b) { return a.size() > b.size(); });
    std::vector<std::string> kept;                  // (one that lies inside a longer one asks nothing more of an entry)
    for (auto &s : distinct) {
        bool inside = false;
        for (auto &t : kept) inside = inside || t.find(s) != std::string::npos;
        if (!inside && kept.size() < REGEX_MAX_LITERALS) kept.push_back(s);
    }
    return kept;
}

// ---- Glushkov positions --------------------------------------------------------------------------------------------
constexpr uint32_t PW = (REGEX_MAX_POSITIONS + 1 + 63) / 64;       // words of a position set (the start marker is position 0)
struct PosSet {
    uint64_t w[PW];
    PosSet() { memset(w, 0, sizeof w); }
    void add(uint32_t q) { w[q >> 6] |= 1ull << (q & 63); }
    bool has(uint32_t q) const { return (w[q >> 6] >> (q & 63)) & 1; }
    // (n: the words in use -- the subset construction knows how many positions there are)
    void merge(const PosSet &o, uint32_t n = PW) { for (uint32_t i = 0; i < n; ++i) w[i] |= o.w[i]; }
    bool meets(const PosSet &o, uint32_t n = PW) const
    {
        for (uint32_t i = 0; i < n; ++i)
            if (w[i] & o.w[i]) return true;
        return false;
    }
    bool none(uint32_t n = PW) const
    {
        for (uint32_t i = 0; i < n; ++i)
            if (w[i]) return false;
        return true;
    }
    template <typename F>
    void each(F f, uint32_t n = PW) const
    {
        for (uint32_t i = 0; i < n; ++i)
            for (uint64_t m = w[i]; m; m &= m - 1) f(i * 64 + (uint32_t)__builtin_ctzll(m));
    }
};

struct Frag {
    bool nullable = true;
    PosSet first, last;
};

struct Glushkov {
    std::vector<ByteSet> chars;                     // per position; [0] is the start marker's
    std::vector<PosSet> follow;
    uint64_t work = 0;                              // fragments built: repeats of repeats of nothing add no position
    Glushkov() : chars(1), follow(1) {}
    void link(const PosSet &from, const PosSet &to) { from.each([&](uint32_t q) { follow[q].merge(to); }); }
    Frag cat(const Frag &a, const Frag &b)
    {
        link(a.last, b.first);
        Frag f;
        f.nullable = a.nullable && b.nullable;
        f.first = a.first;
        if (a.nullable) f.first.merge(b.first);
        f.last = b.last;
        if (b.nullable) f.last.merge(a.last);
        return f;
    }
    Frag build(const Node &nd)
    {
        Frag f;
        if (++work > ((uint64_t)1 << 22)) throw Error{"pattern too complex: its counted repeats unroll into too many pieces"};
        switch (nd.kind) {
        case N_EMPTY: break;
        case N_CHAR: {
            if (chars.size() > REGEX_MAX_POSITIONS)
                throw Error{"pattern too complex: more than " + std::to_string(REGEX_MAX_POSITIONS) + " positions once its counted repeats are unrolled"};
            const uint32_t q = (uint32_t)chars.size();
            chars.push_back(nd.set);
            follow.emplace_back();
            f.nullable = false;
            f.first.add(q);
            f.last.add(q);
            break;
        }
        case N_CAT:
            for (const auto &k : nd.kids) f = cat(f, build(*k));
            break;
        case N_ALT:
            f.nullable = false;
            for (const auto &k : nd.kids) {
                const Frag g = build(*k);
                f.nullable = f.nullable || g.nullable;
                f.first.merge(g.first);
                f.last.merge(g.last);
            }
            break;
        case N_REPEAT: {
            const Node &kid = *nd.kids[0];
            for (uint32_t r = 0; r < nd.lo; ++r) f = cat(f, build(kid));
            if (nd.hi == INF) {
                Frag s = build(kid);
                link(s.last, s.first);
                s.nullable = true;
                f = cat(f, s);
            } else if (nd.hi > nd.lo) {             // (k(k(k)?)?)? -- built from the innermost copy outwards
                Frag tail;
                for (uint32_t r = nd.lo; r < nd.hi; ++r) {
                    tail = cat(build(kid), tail);
                    tail.nullable = true;
                }
                f = cat(f, tail);
            }
            break;
        }
        }
        return f;
    }
};

struct PosSetHash {
    size_t operator()(const std::string &s) const { return std::hash<std::string>()(s); }
};

}  // namespace regex_detail

// pattern[0, len) under `flags` into *out.  true, or false with the reason in *error (a refusal names its position).
inline bool regex_compile(const uint8_t *pattern, uint64_t len, uint32_t flags, RegexDfa *out, std::string *error)
{
    using namespace regex_detail;
    try {
        Parser ps{pattern, len, 0, (flags & REGEX_ICASE) != 0};
        NodeP root = ps.parse();
        RegexDfa d;
        d.anchors = ps.anchors;
        d.literals = required_literals(*root);
        if (d.literals.empty())
            throw Error{"a pattern without a required literal at position 0 (no byte run that every match holds: nothing to look up)"};
        Glushkov G;
        const Frag R = G.build(*root);
        const bool a_start = ps.anchors & REGEX_ANCHOR_START, a_end = ps.anchors & REGEX_ANCHOR_END;
        G.follow[0] = R.first;
        if (!a_start) {                              // the leading [^\n]*: the marker stays while the bytes are no 0x0A
            G.chars[0].add('\n');
            G.chars[0].negate();
            G.follow[0].add(0);
        }
        const uint32_t npos = (uint32_t)G.chars.size(), nw = (npos + 63) / 64;     // positions, and the words of a set that hold them
        PosSet last = R.last;
        if (R.nullable) last.add(0);
        // byte classes: two bytes are one class when every position takes both or neither
        std::vector<ByteSet> sets;
        for (const ByteSet &s : G.chars)
            if (std::find(sets.begin(), sets.end(), s) == sets.end()) sets.push_back(s);
        uint32_t cls[256] = {}, ncls = 1;
        for (const ByteSet &s : sets) {
            int32_t renum[512];                      // (class so far, inside the set or not) -> the class from here on
            std::fill(renum, renum + 512, -1);
            uint32_t next = 0;
            for (uint32_t b = 0; b < 256; ++b) {
                const uint32_t key = cls[b] * 2 + (s.has(b) ? 1 : 0);
                if (renum[key] < 0) renum[key] = (int32_t)next++;
                cls[b] = (uint32_t)renum[key];
            }
            ncls = next;
        }
        std::vector<uint32_t> rep(ncls);
        for (uint32_t b = 256; b-- > 0;) rep[cls[b]] = b;
        std::vector<PosSet> takes(ncls);             // the positions that take a byte of the class
        for (uint32_t q = 0; q < npos; ++q)
            for (uint32_t c = 0; c < ncls; ++c)
                if (G.chars[q].has(rep[c])) takes[c].add(q);
        // subset construction; temporary ids: 0 dead, SINK the absorbing accepting state (no `$`), the rest as discovered
        constexpr uint32_t SINK = 0xffffffffu;
        std::vector<PosSet> states(1);
        std::vector<std::vector<uint32_t>> rows(1, std::vector<uint32_t>(ncls, 0));
        std::unordered_map<std::string, uint32_t> index;
        auto key_of = [&](const PosSet &s) { return std::string(reinterpret_cast<const char *>(s.w), (size_t)nw * 8); };
        auto accepts = [&](const PosSet &s) { return s.meets(last, nw); };
        auto id_of = [&](const PosSet &s) -> uint32_t {
            if (s.none(nw)) return 0;
            if (!a_end && accepts(s)) return SINK;
            auto it = index.find(key_of(s));
            if (it != index.end()) return it->second;
            if (states.size() + (a_end ? 0 : 1) >= REGEX_MAX_STATES)      // (the sink is numbered at the end)
                throw Error{"pattern too complex: its DFA has more than " + std::to_string(REGEX_MAX_STATES) + " states"};
            const uint32_t id = (uint32_t)states.size();
            states.push_back(s);
            rows.emplace_back(ncls, 0);
            index.emplace(key_of(s), id);
            return id;
        };
        PosSet init;
        init.add(0);
        const uint32_t start_tmp = id_of(init);
        for (uint32_t s = 1; s < states.size(); ++s) {
            PosSet next;
            const PosSet cur = states[s];
            cur.each([&](uint32_t q) { next.merge(G.follow[q], nw); }, nw);
            for (uint32_t c = 0; c < ncls; ++c) {
                PosSet to;
                for (uint32_t i = 0; i < nw; ++i) to.w[i] = next.w[i] & takes[c].w[i];
                const uint32_t id = id_of(to);       // (may grow states and rows)
                rows[s][c] = id;
            }
        }
        // final numbers: dead, the states that do not accept, the ones that do (with `$`), the sink (without)
        const uint32_t ntmp = (uint32_t)states.size();
        std::vector<uint32_t> number(ntmp, 0);
        uint32_t next = 1;
        for (uint32_t s = 1; s < ntmp; ++s)
            if (!(a_end && accepts(states[s]))) number[s] = next++;
        d.first_accept = next;
        for (uint32_t s = 1; s < ntmp; ++s)
            if (a_end && accepts(states[s])) number[s] = next++;
        if (!a_end) d.sink = next++;
        d.nstates = next;
        d.ncls = ncls;
        for (uint32_t b = 0; b < 256; ++b) d.cls[b] = (uint8_t)cls[b];
        d.table.assign((size_t)d.nstates * ncls, 0);
        auto final_of = [&](uint32_t tmp) { return tmp == SINK ? d.sink : number[tmp]; };
        for (uint32_t s = 1; s < ntmp; ++s)
            for (uint32_t c = 0; c < ncls; ++c) d.table[(size_t)number[s] * ncls + c] = (uint16_t)final_of(rows[s][c]);
        if (!a_end)
            for (uint32_t c = 0; c < ncls; ++c) d.table[(size_t)d.sink * ncls + c] = (uint16_t)d.sink;
        d.start = final_of(start_tmp);
        *out = std::move(d);
        return true;
    } catch (const regex_detail::Error &e) {
        *error = e.msg;
        return false;
    }
}

}  // namespace pss
