"""Seeded cases for the differential fuzz of every entry-level search kind (entry ids, anchored, all-terms, wildcard,
case-insensitive): inputs that nobody designed, for the brute-force references of tests/*_ref.py to judge.

make_case(seed) is a pure function of the seed (random.Random(seed) through randrange and random alone; no clock, no
numpy state) and returns a Case: the entries, the chunk texts they lie in, how the reader is to be opened, the search
switches to set, and one batch per kind of about PER_BATCH patterns.  CPU only; tests/test_search_fuzz_cases.py judges
the generator and the references with it, tests/test_search_fuzz_gpu.py and tests/tools/fuzz_search.py run the engine
on it.

What is drawn, and why these values (the in-entry scan works on 8-byte words, 8 lanes to a 64-byte step):
  * one alphabet per case: two symbols (every piece occurs many times per entry), mixed case of few letters, the edges of
    the fold ('@' 'A' 'Z' '[' and '`' 'a' 'z' '{'), bytes that differ by 0x20 and are no letters together with 0x00, the
    glob metacharacters as data, one wide printable alphabet;
  * entry lengths from LENGTHS -- around the word and the step, three steps plus a tail -- never from a uniform range;
  * entry bodies: words of a small per-case pool back to back, one word repeated, symbols at random;
  * 1, 3, 40 or 300 entries in about 1, 2 or 5 chunks, cut by the Writer's own rule (a chunk is closed when the next
    entry and its newline would pass max_chunk_len); sometimes the last chunk lacks its closing newline, and such a case
    is handed over on the device;
  * patterns cut from a drawn entry so that they hit, a share of them near misses (one byte changed, neighbours
    swapped, a piece of another entry, the last segment doubled, two segments that overlap by one byte)."""
import random
import typing

from pysubstringsearch_amd import glob_escape

SEEDS = range(24)
PER_BATCH = 40
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 56, 63, 64, 65, 71, 72, 73, 127, 128, 129, 200)
ALPHABETS = (b'ab', b'abAB', b'aAzZ@[`{', b'\x00a\xc1\xe1A', b'a*\\b', bytes(range(0x20, 0x7f)))
PIECE_LENS = (1, 2, 7, 8, 9, 16, 64, 200)
KINDS = ('start', 'end', 'entry')
SETUPS = ('file', 'devices', 'shard', 'host', 'sa', 'device')
START, END = 1, 2


class Case(typing.NamedTuple):
    seed: int
    alphabet: bytes
    entries: typing.List[bytes]
    chunks: typing.List[bytes]                  # the chunk texts: the entries with their newlines, in order
    max_chunk_len: typing.Optional[int]         # the Writer's argument that cuts the file into `chunks`
    closed: bool                                # False: the last chunk has no closing newline (setup == 'device')
    setup: str                                  # one of SETUPS
    shard: typing.Optional[typing.Tuple[int, int]]
    switches: typing.Dict[str, int]             # PSS_* search switches to set before the reader is opened
    ids: typing.List[bytes]
    anchored: typing.List[typing.Tuple[bytes, str]]
    anchored_word: typing.Tuple[typing.List[bytes], str]        # one batch under ONE anchor word
    all_terms: typing.List[typing.Tuple[typing.List[bytes], typing.List[bytes]]]
    glob: typing.List[typing.Tuple[typing.List[bytes], int, bytes]]        # (segments, anchors, the pattern's bytes)
    icase: typing.List[bytes]

    @property
    def interval(self) -> typing.Optional[str]:
        """The interval route the switches fix ('INTERVAL_WAVE' / 'INTERVAL_LANE'), or None: it follows the batch."""
        if self.switches.get('PSS_WAVE_SEARCH'):
            return 'INTERVAL_WAVE'
        return 'INTERVAL_LANE' if self.switches.get('PSS_LANE_SEARCH_MIN') == 1 else None


def case_bytes(case: Case) -> bytes:
    """Everything a case holds as one byte string (what the pinned hash is taken over)."""
    return repr((tuple(case[:8]), sorted(case.switches.items()), tuple(case[9:]))).encode()


def glob_pattern(segments: typing.Sequence[bytes], anchors: int) -> bytes:
    """The glob pattern of (segments, anchors), as tests/test_glob_gpu.glob() writes it."""
    p = b'*'.join(glob_escape(s) for s in segments)
    return (b'' if anchors & START else b'*') + p + (b'' if anchors & END else b'*')


def is_letter(b: int) -> bool:
    return 0x41 <= (b & ~0x20) <= 0x5A


class _Draw:
    """The few draws everything is made of: randrange and random keep their meaning across Python versions."""

    def __init__(self, seed: int):
        self.r = random.Random(seed)

    def below(self, n: int) -> int:
        return self.r.randrange(n)

    def between(self, lo: int, hi: int) -> int:
        return lo + self.r.randrange(hi - lo + 1)

    def pick(self, seq):
        return seq[self.r.randrange(len(seq))]

    def chance(self, p: float) -> bool:
        return self.r.random() < p

    def symbols(self, alphabet: bytes, n: int) -> bytes:
        return bytes(alphabet[self.r.randrange(len(alphabet))] for _ in range(n))

    def cuts(self, n: int, k: int) -> typing.List[int]:
        """k distinct positions of 0 .. n, ascending (k <= n + 1)."""
        got = set()
        while len(got) < k:
            got.add(self.r.randrange(n + 1))
        return sorted(got)


def chunk_texts(entries: typing.Sequence[bytes], limit: typing.Optional[int]) -> typing.List[bytes]:
    """The chunks the Writer cuts a file of these entries into: an entry that would take the chunk past `limit` bytes
    with its newline opens the next one (limit >= every entry's length + 1, so the limit never grows)."""
    if limit is None:
        return [b''.join(e + b'\n' for e in entries)]
    out, cur = [], bytearray()
    for e in entries:
        assert len(e) + 1 <= limit
        if len(cur) + len(e) + 1 > limit:
            out.append(bytes(cur))
            cur = bytearray()
        cur += e + b'\n'
    out.append(bytes(cur))
    return out


def _entries(d: _Draw, alphabet: bytes, count: int) -> typing.List[bytes]:
    pool = [d.symbols(alphabet, d.between(1, 9)) for _ in range(d.between(2, 6))]
    out = []
    for _ in range(count):
        n, style = d.pick(LENGTHS), d.below(3)
        if style == 0:                              # words of the pool, back to back
            body = b''
            while len(body) < n:
                body += d.pick(pool)
        elif style == 1:                            # one word repeated
            w = d.pick(pool)
            body = w * (n // len(w) + 1)
        else:
            body = d.symbols(alphabet, n)
        out.append(body[:n])
    return out


class _Patterns:
    def __init__(self, d: _Draw, alphabet: bytes, entries: typing.Sequence[bytes]):
        self.d, self.alphabet = d, alphabet
        self.entries = list(entries)
        self.filled = [e for e in entries if e]

    def entry(self, min_len: int = 1) -> bytes:
        """A drawn entry of at least min_len bytes -- or, where the case has none, symbols at random."""
        fit = [e for e in self.filled if len(e) >= min_len]
        return self.d.pick(fit) if fit else self.d.symbols(self.alphabet, max(1, min_len))

    def piece(self, e: typing.Optional[bytes] = None, n: typing.Optional[int] = None) -> bytes:
        e = self.entry() if e is None else e
        n = min(len(e), self.d.pick((1, 1, 2, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 30, 64)) if n is None else n)
        at = self.d.below(len(e) - n + 1)
        return e[at:at + n]

    def changed(self, b: bytes, by_0x20: bool = False) -> bytes:
        """b with one byte changed: to another symbol of the alphabet, or (by_0x20, where b has such a byte) a byte that
        is no letter to the one 0x20 away -- what a fold that is too wide takes for the same."""
        at = self.d.below(len(b))
        if by_0x20:
            odd = [i for i, x in enumerate(b) if not is_letter(x) and x ^ 0x20 != 0x0A]
            if odd:
                at = self.d.pick(odd)
                return b[:at] + bytes([b[at] ^ 0x20]) + b[at + 1:]
        x = self.d.pick([s for s in self.alphabet if s != b[at]])
        return b[:at] + bytes([x]) + b[at + 1:]

    def ids(self) -> bytes:
        p = self.piece()
        return self.changed(p) if self.d.chance(0.25) else p

    def anchored(self) -> typing.Tuple[bytes, str]:
        d, e = self.d, self.entry()
        n = d.pick([m for m in PIECE_LENS if m <= len(e)])
        how = d.below(20)
        if how < 5:                                 # a prefix, mostly asked for as one
            return e[:n], 'start' if d.chance(0.7) else d.pick(KINDS)
        if how < 10:
            return e[len(e) - n:], 'end' if d.chance(0.7) else d.pick(KINDS)
        if how < 13:
            return e, 'entry' if d.chance(0.7) else d.pick(KINDS)
        if how < 17:                                # an inner piece: it occurs, and is not anchored
            return self.piece(e, n), d.pick(KINDS)
        return self.changed(e), d.pick(KINDS)       # a whole entry with one byte changed

    def all_terms(self) -> typing.Tuple[typing.List[bytes], typing.List[bytes]]:
        d, e = self.d, self.entry()
        include = [self.piece(e) for _ in range(d.between(1, 5))]
        if d.chance(0.25):
            include[d.below(len(include))] = self.piece()
        exclude = [self.piece() for _ in range(d.pick((0, 0, 0, 1, 1, 2)))]
        return include, exclude

    def glob(self) -> typing.Tuple[typing.List[bytes], int, bytes]:
        d, e = self.d, self.entry()
        k = min(d.between(1, 4), max(1, len(e) // 2))
        if d.chance(0.4) and len(e) >= k:           # adjacent segments: every gap is zero
            c = d.cuts(len(e), k + 1)
            spans = [(c[i], c[i + 1]) for i in range(k)]
        else:
            c = d.cuts(len(e), 2 * k) if len(e) + 1 >= 2 * k else [0, len(e)]
            spans = [(c[2 * i], c[2 * i + 1]) for i in range(len(c) // 2)]
        anchors = d.pick((0, 0, 0, 0, 1, 1, 2, 2, 3, 3))
        if anchors & START and d.chance(0.7):       # the first segment from the entry's true start
            spans[0] = (0, spans[0][1])
        if anchors & END and d.chance(0.7):
            spans[-1] = (spans[-1][0], len(e))
        segs = [e[a:b] for a, b in spans if a < b] or [e[:1]]
        how = d.below(20)
        if how < 3 and len(segs) >= 2:              # two neighbours swapped
            at = d.below(len(segs) - 1)
            segs[at], segs[at + 1] = segs[at + 1], segs[at]
        elif how < 5:
            at = d.below(len(segs))
            segs[at] = self.changed(segs[at])
        elif how < 8 and len(segs) < 8:             # the last segment twice: it has to occur again, behind itself
            segs.append(segs[-1])
        elif how < 11 and len(spans) >= 2 and len(segs) == len(spans):
            at = d.between(1, len(spans) - 1)       # a segment that begins on the last byte of the one before it
            before = spans[at - 1][1]
            segs[at] = e[before - 1:max(spans[at][1], before)]
        return segs, anchors, glob_pattern(segs, anchors)

    def icase(self) -> bytes:
        d = self.d
        p = self.piece(n=d.between(1, 30))
        p = bytes(x ^ 0x20 if is_letter(x) and d.chance(0.5) else x for x in p)
        return self.changed(p, by_0x20=d.chance(0.5)) if d.chance(0.25) else p


def make_case(seed: int) -> Case:
    d = _Draw(seed)
    alphabet = d.pick(ALPHABETS)
    entries = _entries(d, alphabet, d.pick((1, 3, 40, 300)))
    # chunks: the limit that gives about the drawn number, never below the longest entry with its newline
    want = d.pick((1, 2, 5))
    total = sum(len(e) + 1 for e in entries)
    limit = None if want == 1 else max(-(-total // want), max(len(e) for e in entries) + 1)
    chunks = chunk_texts(entries, limit)
    setup = d.pick(SETUPS)
    closed = True
    if d.chance(0.25) and entries[-1]:              # (an empty last entry without its newline is no entry at all)
        setup, closed = 'device', False
        chunks[-1] = chunks[-1][:-1]
    shard = None
    if setup == 'shard':
        n = d.pick((2, 3))
        shard = (d.below(min(n, len(chunks))), n)   # a rank that holds a chunk
    sw: typing.Dict[str, int] = {}
    route = d.below(4)
    if route == 1:
        sw['PSS_LANE_SEARCH_MIN'] = 1
    elif route == 2:
        sw['PSS_LANE_SEARCH_MIN'] = 100000
    elif route == 3:
        sw['PSS_WAVE_SEARCH'] = 1
    for name in ('PSS_NO_GROUP_SEARCH', 'PSS_NO_SEARCH_STAGE', 'PSS_NO_PINNED_RESULTS', 'PSS_NO_MID_PIPELINE'):
        if d.chance(0.3):
            sw[name] = 1
    x = d.r.random()
    if x < 0.15:
        sw['PSS_NO_KEY_SAMPLES'] = 1
    elif x < 0.85:
        sw['PSS_SAMPLE_SHIFT'] = d.between(0, 8)
    if d.chance(0.6):
        sw['PSS_ICASE_SEED_LETTERS'] = d.between(1, 6)
    p = _Patterns(d, alphabet, entries)
    word = d.pick(KINDS)
    word_batch = []
    for _ in range(PER_BATCH):
        e = p.entry()
        n = d.pick([m for m in PIECE_LENS if m <= len(e)])
        piece = e if word == 'entry' and d.chance(0.5) else e[:n] if word == 'start' else e[len(e) - n:] if word == 'end' else p.piece(e, n)
        word_batch.append(p.changed(piece) if d.chance(0.2) else piece)
    return Case(seed, alphabet, entries, chunks, limit, closed, setup, shard, sw,
                ids=[p.ids() for _ in range(PER_BATCH)],
                anchored=[p.anchored() for _ in range(PER_BATCH)],
                anchored_word=(word_batch, word),
                all_terms=[p.all_terms() for _ in range(PER_BATCH)],
                glob=[p.glob() for _ in range(PER_BATCH)],
                icase=[p.icase() for _ in range(PER_BATCH)])
