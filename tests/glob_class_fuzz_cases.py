"""Seeded cases for the differential fuzz of the wildcard search with byte classes: inputs that nobody designed, for the
brute-force reference of tests/glob_class_ref.py to judge.

make_case(seed) is a pure function of the seed.  The corpus, the way the reader is opened and the PSS_* switches are those
of tests/search_fuzz_cases.make_case(seed) -- 1 .. 300 entries over alphabets that hold the glob metacharacters, 0x00 and
bytes >= 0x80 as data, 1 .. 5 chunks, every reader placement --; on top come PER_BATCH class patterns of a Random(seed) of
their own.  A pattern is cut from ONE drawn entry, left to right, as the plain glob cases are, and then every byte of a
piece stays a literal (escaped), or becomes `?`, a set that holds it (members one by one or as a range around it) or a
negated set that does not; one piece in three loses every literal (a coreless segment) where another keeps one.  Pattern
i is written under anchor byte i % 4, so every case holds all four.  One pattern in five is a near miss: one class
position that rejects the entry's byte, a `?` too many, or two pieces swapped.  CPU only;
tests/test_glob_class_host.py judges the generator, tests/test_glob_class_fuzz_gpu.py runs the engine on it."""
import random
import typing

from tests import search_fuzz_cases as base

SEEDS = (0, 1, 3, 4, 5, 8, 9, 10, 12, 14, 18, 20)     # every placement; none whose corpus is one entry of one byte
PER_BATCH = 24
START, END = 1, 2


class Case(typing.NamedTuple):
    seed: int
    entries: typing.List[bytes]
    chunks: typing.List[bytes]
    max_chunk_len: typing.Optional[int]
    closed: bool
    setup: str
    shard: typing.Optional[typing.Tuple[int, int]]
    switches: typing.Dict[str, int]
    interval: typing.Optional[str]
    patterns: typing.List[bytes]
    glob: typing.List[bytes]                    # plain glob patterns of the same corpus (tests/search_fuzz_cases.py)


def _lit(b: int) -> bytes:
    return b'\\' + bytes([b])


def _set_with(rnd: random.Random, alphabet: bytes, b: int) -> bytes:
    if rnd.random() < 0.4:                      # a range around the byte
        lo, hi = max(0, b - rnd.randrange(0, 3)), min(255, b + rnd.randrange(0, 3))
        return b'[' + _lit(lo) + b'-' + _lit(hi) + b']'
    members = [b] + [rnd.choice(alphabet) for _ in range(rnd.randrange(0, 3))]
    rnd.shuffle(members)
    return b'[' + b''.join(_lit(m) for m in members) + b']'


def _set_without(rnd: random.Random, alphabet: bytes, b: int, negate: bool = True) -> bytes:
    fold = b ^ 0x20 if 0x41 <= (b & 0xDF) <= 0x5A else b           # (not the byte's other case either: the pattern is run under fold too)
    others = [x for x in alphabet if x not in (b, fold, 0x0A)] or [b ^ 0xFF]
    members = [rnd.choice(others) for _ in range(rnd.randrange(1, 4))]
    return (b'[!' if negate else b'[') + b''.join(_lit(m) for m in members) + b']'


def _piece(rnd: random.Random, alphabet: bytes, text: bytes, coreless: bool) -> typing.List[bytes]:
    """One segment over the bytes of text, position by position."""
    out = []
    for b in text:
        roll = rnd.random()
        if coreless:
            roll = 0.5 + roll / 2
        if roll < 0.5:
            out.append(_lit(b))
        elif roll < 0.7:
            out.append(b'?')
        elif roll < 0.85:
            out.append(_set_with(rnd, alphabet, b))
        else:
            out.append(_set_without(rnd, alphabet, b))
    return out


def _pattern(rnd: random.Random, alphabet: bytes, entries: typing.Sequence[bytes], anchors: int, coreless: bool, miss: bool) -> bytes:
    e = rnd.choice(entries)
    k = min(rnd.choice((1, 2, 2, 3, 4)), max(1, len(e) // 2))
    cuts = sorted(rnd.sample(range(len(e) + 1), min(2 * k, len(e) + 1)))
    cuts = cuts[:len(cuts) // 2 * 2]
    if anchors & START:
        cuts[0] = 0
    if anchors & END:
        cuts[-1] = len(e)
    spans = [(cuts[i], cuts[i + 1]) for i in range(0, len(cuts), 2) if cuts[i] < cuts[i + 1]] or [(0, len(e))]
    if coreless and len(spans) == 1:            # two adjacent pieces, so that one of them can do without a literal
        a, b = spans[0] if spans[0][1] - spans[0][0] >= 2 else (0, len(e))
        m = rnd.randrange(a + 1, b)
        spans = [(a, m), (m, b)]
    bare = rnd.randrange(len(spans)) if coreless else -1
    segs = [_piece(rnd, alphabet, e[a:b], i == bare) for i, (a, b) in enumerate(spans)]
    if not any(p.startswith(b'\\') for s in segs for p in s):        # a pattern needs a literal byte
        at = next(i for i in range(len(segs)) if i != bare)
        segs[at][0] = _lit(e[spans[at][0]])
    if miss:
        how = rnd.randrange(3)
        at = rnd.randrange(len(segs))
        if how == 0:                            # a class position that rejects the entry's byte there
            i = rnd.randrange(len(segs[at]))
            b = e[spans[at][0] + i]
            if rnd.random() < 0.5:
                segs[at][i] = b'[!' + _lit(b) + b']'
            else:
                segs[at][i] = _set_without(rnd, alphabet, b, negate=False)
        elif how == 1:                          # one byte more than the cut has room for
            segs[at].insert(rnd.randrange(len(segs[at]) + 1), b'?')
        elif len(segs) > 1:
            at = rnd.randrange(len(segs) - 1)
            segs[at], segs[at + 1] = segs[at + 1], segs[at]
    if not any(p.startswith(b'\\') for s in segs for p in s):
        segs[0][0] = _lit(e[spans[0][0]])
    body = b'*'.join(b''.join(s) for s in segs)
    return (b'' if anchors & START else b'*') + body + (b'' if anchors & END else b'*')


def make_case(seed: int) -> Case:
    c = base.make_case(seed)
    rnd = random.Random(seed)
    full = [e for e in c.entries if len(e) >= 2 and b'\n' not in e] or [bytes(c.alphabet[:2]) or b'ab']
    patterns = [_pattern(rnd, c.alphabet, full, i % 4, coreless=i % 3 == 0, miss=i % 5 == 4) for i in range(PER_BATCH)]
    return Case(seed, c.entries, c.chunks, c.max_chunk_len, c.closed, c.setup, c.shard, c.switches, c.interval, patterns,
                [g for _, _, g in c.glob])
