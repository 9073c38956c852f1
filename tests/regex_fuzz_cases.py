"""Seeded cases for the differential fuzz of the regular-expression search: the texts, chunks, reader set-ups and switches
of tests/search_fuzz_cases.py (make_case(seed), unchanged) with two batches of regular expressions drawn on top, one for
exact bytes and one for icase=True, and (pattern, string) pairs for the host matcher.

make_regex_case(seed) is a pure function of the seed.  Every pattern stays inside the subset the engine takes (include/pss.h,
pss_regex_compile) and is built around an entry: pieces of the entry as literals, the bytes between them as something that
takes them -- `.*`, `.{k}`, a counted set of their bytes, a negated set of a byte they lack, `\\w*` and its kin where they
fit, an alternation, an optional group -- and `^` / `$` with what stands before the first and behind the last piece.  A share
are near misses: two pieces swapped (the literals are all there, in the wrong order), a count one off, a byte of a piece
changed, a set that lacks one byte of its gap.  The alphabets hold 0x00 and bytes >= 0x80.  CPU only."""
import re
import typing

from tests.search_fuzz_cases import Case, _Draw, _Patterns, is_letter, make_case

SEEDS = range(24)
PER_BATCH = 40
COUNT_MAX = 6           # the largest count a drawn gap is written with
SPECIAL = b'\\.^$*+?{}[]()|'


class RegexCase(typing.NamedTuple):
    base: Case                                  # entries, chunks, set-up and switches
    regex: typing.List[bytes]
    regex_icase: typing.List[bytes]
    pairs: typing.List[typing.Tuple[bytes, bytes, bool]]        # (pattern, string without 0x0A, icase) for the host matcher


def esc(b: bytes) -> bytes:
    """b as a pattern that matches exactly these bytes (the package's regex_escape, restated)."""
    return b''.join(b'\\' + bytes([x]) if x in SPECIAL else bytes([x]) for x in b)


def hexed(x: int) -> bytes:
    return b'\\x%02x' % x


class _Regexes(_Patterns):
    def gap(self, g: bytes, miss: bool = False) -> bytes:
        """Something that takes the bytes g (miss: that fails on them where it can)."""
        d = self.d
        if miss and g:
            if d.chance(0.5) and len(g) < COUNT_MAX:
                return b'.{%d}' % (len(g) + 1)
            lack = d.pick(sorted(set(g)))
            return b'[^%s]*' % hexed(lack)
        if not g:
            return d.pick((b'', b'', b'.*', b'(?:%s)?' % esc(self.piece(n=2)), b'\\d*', b'.{0,3}'))
        how = d.below(10)
        if len(g) > COUNT_MAX and how in (1, 2, 8):     # (a long counted gap behind an unanchored literal: 2^k DFA states)
            how = 0 if how == 1 else 3
        if how == 0:
            return b'.*'
        if how == 1:
            return b'.{%d}' % len(g)
        if how == 2:
            return b'.{%d,%d}' % (d.between(0, len(g)), len(g) + d.between(0, 2))
        if how == 3:
            return b'[%s]%s' % (b''.join(hexed(x) for x in sorted(set(g))), d.pick((b'+', b'*', b'{%d}' % len(g) if len(g) <= COUNT_MAX else b'+', b'{1,}')))
        if how == 4:
            absent = [x for x in range(256) if x not in g and x != 0x0A]
            return b'[^%s\\n]%s' % (hexed(d.pick(absent)), d.pick((b'+', b'*')))
        if how == 5:
            for cls in (b'\\w+', b'\\S+', b'\\D*', b'\\W+', b'[a-zA-Z]+', b'[\\x00-\\x7f]*'):
                if re.fullmatch(cls, g):
                    return cls
            return b'.+'
        if how == 6:
            other = self.piece(n=d.between(1, 4))
            alts = [esc(g), esc(other)]
            if d.chance(0.5):
                alts.reverse()
            return b'(' + b'|'.join(alts) + b')'
        if how == 7 and len(g) <= 8:
            return b'(?:' + esc(g) + b')' + d.pick((b'+', b'{1,2}', b'{1}'))
        if how == 8:
            return b'(' + esc(g[:1]) + b'|.)' + (b'.{%d}' % (len(g) - 1) if len(g) > 1 else b'')
        return b'.*' + esc(g[-1:]) if d.chance(0.5) else b'.+'

    def regex(self, icase: bool = False) -> bytes:
        d, e = self.d, self.entry(2)
        k = min(d.between(1, 3), max(1, len(e) // 2))
        c = d.cuts(len(e), 2 * k) if len(e) + 1 >= 2 * k else [0, len(e)]
        spans = [(c[2 * i], c[2 * i + 1]) for i in range(len(c) // 2)]
        spans = [(a, b) for a, b in spans if a < b] or [(0, 1)]
        how = d.below(20)
        lits = [e[a:b] for a, b in spans]
        if icase:
            lits = [bytes(x ^ 0x20 if is_letter(x) and d.chance(0.5) else x for x in lit) for lit in lits]
        gaps = [e[spans[i][1]:spans[i + 1][0]] for i in range(len(spans) - 1)]
        miss_gap = -1
        if how < 3 and len(lits) >= 2:              # two neighbours swapped: every literal is there, the order is wrong
            at = d.below(len(lits) - 1)
            lits[at], lits[at + 1] = lits[at + 1], lits[at]
        elif how < 5:
            at = d.below(len(lits))
            lits[at] = self.changed(lits[at])
        elif how < 9 and gaps:
            miss_gap = d.below(len(gaps))
        out = b''
        anchors = d.pick((0, 0, 0, 1, 2, 3))
        if anchors & 1:
            out += b'^' + self.gap(e[:spans[0][0]], miss=how == 9)
        for i, lit in enumerate(lits):
            out += esc(lit)
            if i < len(gaps):
                out += self.gap(gaps[i], miss=i == miss_gap)
        if anchors & 2:
            out += self.gap(e[spans[-1][1]:], miss=how == 10) + b'$'
        self.source = e
        return out

    def strings(self, e: bytes) -> typing.List[bytes]:
        """What a pattern built around the entry e is tried on: e, e with a byte changed, another entry, symbols at random."""
        return [e, self.changed(e), self.entry(), self.d.symbols(self.alphabet, self.d.between(0, 20))]


def make_regex_case(seed: int) -> RegexCase:
    base = make_case(seed)
    d = _Draw(7000 + seed)
    p = _Regexes(d, base.alphabet, base.entries)
    rx, rxi, pairs = [], [], []
    for batch, fold in ((rx, False), (rxi, True)):
        for _ in range(PER_BATCH):
            batch.append(p.regex(icase=fold))
            pairs += [(batch[-1], s, fold) for s in p.strings(p.source)]
    return RegexCase(base, rx, rxi, pairs)
