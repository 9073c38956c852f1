"""Seeded cases for the differential fuzz of the case-insensitive all-terms and wildcard search: inputs that nobody
designed, for the brute-force reference of tests/icase_groups_ref.py to judge.

make_case(seed) is a pure function of the seed (random.Random(seed) alone; no clock, no numpy state) and returns a Case:
a small case-mangled corpus (at most 64 KiB) cut into 1 .. 4 chunk texts by the Writer's own rule, the last of them
sometimes without its closing newline (the chunks are handed over on the device), the PSS_ICASE_SEED_LETTERS to set, and
PER_BATCH all-terms groups and PER_BATCH glob patterns drawn from the corpus.  CPU only;
tests/test_icase_groups_fuzz_cases.py judges the generator and the reference with it, tests/test_icase_groups_fuzz_gpu.py
runs the engine on it.

What is drawn:
  * one alphabet per case -- few letters in both cases; letters, digits and the bytes beside the letters ('@' '[' '`' '{');
    bytes that differ by 0x20 and are no letters, with 0x00 and bytes >= 0x80; the glob metacharacters as data -- and from
    it a pool of words whose lengths sit around the 8-byte word of the in-entry scan;
  * entries of 0 .. 7 words, with or without blanks between them, the case of every letter flipped at random;
  * include terms cut from ONE drawn entry (the group hits), or from several (it mostly does not); a short, common term in
    front of a longer one, so that the driver is not always the first term; exclude terms from the pool;
  * glob segments cut from one entry left to right, under every anchor byte; near misses: two segments swapped, one
    byte changed, an anchor the cut does not support."""
import random
import typing

from pysubstringsearch_amd import glob_escape

SEEDS = range(16)
PER_BATCH = 20
ALPHABETS = (b'abAB', b'abcxyz019@[`{', b'aZ\x00 \xc1\xe1@`', b'ab*\\Q', b'qrstuvwxyz')
WORD_LENS = (1, 2, 3, 5, 7, 8, 9, 12, 17)
LETTERS = (None, 1, 3, 6)
START, END = 1, 2


class Case(typing.NamedTuple):
    seed: int
    entries: typing.List[bytes]
    chunks: typing.List[bytes]                  # the chunk texts: the entries with their newlines, in order
    closed: bool                                # False: the last chunk has no closing newline
    letters: typing.Optional[int]               # PSS_ICASE_SEED_LETTERS, or None for the default
    groups: typing.List[typing.Tuple[typing.List[bytes], typing.List[bytes]]]
    globs: typing.List[bytes]


def mangle(rnd: random.Random, b: bytes, p: float = 0.5) -> bytes:
    return bytes(c ^ 0x20 if (c | 0x20) in range(0x61, 0x7b) and rnd.random() < p else c for c in b)


def chunk_texts(entries: typing.Sequence[bytes], limit: int) -> typing.List[bytes]:
    """The Writer's rule: a chunk is closed when the next entry and its newline would pass the limit."""
    chunks, cur = [], b''
    for e in entries:
        if cur and len(cur) + len(e) + 1 > limit:
            chunks.append(cur)
            cur = b''
        cur += e + b'\n'
    if cur:
        chunks.append(cur)
    return chunks


def _cut(rnd: random.Random, e: bytes, lo: int = 1, hi: int = 9) -> bytes:
    n = min(len(e), rnd.randrange(lo, hi + 1))
    at = rnd.randrange(0, len(e) - n + 1)
    return e[at:at + n]


def make_case(seed: int) -> Case:
    rnd = random.Random(seed)
    alphabet = ALPHABETS[seed % len(ALPHABETS)]
    pool = [bytes(rnd.choice(alphabet) for _ in range(rnd.choice(WORD_LENS))) for _ in range(rnd.choice((4, 8, 14)))]
    entries = []
    for _ in range(rnd.choice((40, 150, 400))):
        words = [rnd.choice(pool) for _ in range(rnd.randrange(0, 8))]
        entries.append(mangle(rnd, (b' ' if rnd.random() < 0.7 else b'').join(words)))
    total = sum(len(e) + 1 for e in entries)
    assert total <= 65536
    chunks = chunk_texts(entries, max(64, total // rnd.choice((1, 2, 3, 4)) + 1))[:4]
    kept = sum(c.count(b'\n') for c in chunks)
    entries = entries[:kept]
    closed = rnd.random() < 0.6 or not entries[-1]
    if not closed:
        chunks[-1] = chunks[-1][:-1]
    full = [e for e in entries if len(e) >= 4] or [b'abcd']

    groups = []
    while len(groups) < PER_BATCH:
        roll = rnd.random()
        e = rnd.choice(full)
        k = rnd.randrange(1, 4)
        if roll < 0.8:                          # every include term from one entry
            include = [_cut(rnd, e) for _ in range(k)]
        else:                                   # ... or from several
            include = [_cut(rnd, rnd.choice(full)) for _ in range(k)]
        if rnd.random() < 0.5:                  # a short term in front of the others
            include.insert(0, _cut(rnd, e, 1, 2))
        exclude = [_cut(rnd, rnd.choice(pool), 3, 8) for _ in range(rnd.choice((0, 0, 0, 1, 1, 2)))]
        clean = lambda ts: [mangle(rnd, t) for t in ts if t and b'\n' not in t]
        include, exclude = clean(include), clean(exclude)
        if include:
            groups.append((include, exclude))

    globs = []
    while len(globs) < PER_BATCH:
        e = rnd.choice(full)
        k = min(rnd.choice((1, 2, 2, 3, 4)), len(e))
        cuts = sorted(rnd.sample(range(len(e) + 1), min(2 * k, len(e) + 1)))
        cuts = cuts[:len(cuts) // 2 * 2]
        segs = [e[cuts[i]:cuts[i + 1]] for i in range(0, len(cuts), 2)]
        segs = [s for s in segs if s]
        if not segs:
            continue
        anchors = (START if cuts[0] == 0 and rnd.random() < 0.7 else 0) | (END if cuts[-1] == len(e) and rnd.random() < 0.7 else 0)
        roll = rnd.random()
        if roll < 0.12 and len(segs) > 1:       # near misses
            i = rnd.randrange(len(segs) - 1)
            segs[i], segs[i + 1] = segs[i + 1], segs[i]
        elif roll < 0.24:
            i = rnd.randrange(len(segs))
            segs[i] = segs[i][:-1] + bytes([segs[i][-1] ^ 0x01])
        elif roll < 0.36:
            anchors = rnd.randrange(1, 4)
        if any(b'\n' in s for s in segs):
            continue
        body = b'*'.join(glob_escape(mangle(rnd, s)) for s in segs)
        globs.append((b'' if anchors & START else b'*') + body + (b'' if anchors & END else b'*'))
    return Case(seed, entries, chunks, closed, LETTERS[(seed // len(ALPHABETS)) % len(LETTERS)], groups, globs)
