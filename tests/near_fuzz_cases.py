"""Seeded cases for the differential fuzz of the search within k mismatches: inputs that nobody designed, for the
brute-force reference of tests/near_ref.py to judge.

make_case(seed) is a pure function of the seed (the _Draw of tests/search_fuzz_cases.py: random.Random(seed) through
randrange and random alone) and returns a Case: the entries, the chunk texts they lie in, how the reader is to be opened,
and one batch of PER_BATCH (pattern, k) pairs.  CPU only; tests/test_near_fuzz_cases.py judges the generator and the
reference with it, tests/test_near_fuzz_gpu.py runs the engine on it.

What is drawn:
  * one alphabet per case: two, three or four letters -- every piece occurs many times per entry, pieces repeat and nest,
    and a window within budget is never far -- or 0x00 with bytes >= 0x80;
  * entry lengths from search_fuzz_cases.LENGTHS (around the 8-byte word and the 64-byte step of the in-entry scan), and
    the entry bodies of that file: words of a small pool back to back, one word repeated, symbols at random;
  * 3, 40 or 150 entries in about 1, 2 or 4 chunks, cut by the Writer's own rule; sometimes the last chunk lacks its
    closing newline, and such a case is handed over on the device;
  * k 0 .. 3 per pattern; patterns of k + 1 .. 26 bytes cut from the CHUNK TEXT -- a cut that spans a newline gets a symbol
    in the newline's place, which leaves a window within budget that reaches over the newline -- and given 0 .. k + 1
    substitutions at drawn positions."""
import typing

from tests.search_fuzz_cases import LENGTHS, _Draw, _entries, chunk_texts

SEEDS = range(20)
PER_BATCH = 24
ALPHABETS = (b'ab', b'abc', b'abcd', b'\x00a\xc1\xff')
PATTERN_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 26)
SETUPS = ('file', 'devices', 'shard', 'host', 'device')
assert LENGTHS[0] == 0 and max(LENGTHS) == 200


class Case(typing.NamedTuple):
    seed: int
    alphabet: bytes
    entries: typing.List[bytes]
    chunks: typing.List[bytes]                  # the chunk texts: the entries with their newlines, in order
    max_chunk_len: typing.Optional[int]         # the Writer's argument that cuts the file into `chunks`
    closed: bool                                # False: the last chunk has no closing newline (setup == 'device')
    setup: str                                  # one of SETUPS
    shard: typing.Optional[typing.Tuple[int, int]]
    patterns: typing.List[bytes]
    budgets: typing.List[int]


def make_case(seed: int) -> Case:
    d = _Draw(1000 + seed)
    alphabet = ALPHABETS[seed % len(ALPHABETS)]
    entries = _entries(d, alphabet, d.pick((3, 40, 150)))
    want = d.pick((1, 2, 4))
    total = sum(len(e) + 1 for e in entries)
    limit = None if want == 1 else max(-(-total // want), max(len(e) for e in entries) + 1)
    chunks = chunk_texts(entries, limit)
    setup = SETUPS[(seed // len(ALPHABETS)) % len(SETUPS)]
    closed = True
    if setup == 'device' and entries[-1] and d.chance(0.7):       # (an empty last entry without its newline is no entry at all)
        closed = False
        chunks[-1] = chunks[-1][:-1]
    shard = None
    if setup == 'shard':
        n = d.pick((2, 3))
        shard = (d.below(min(n, len(chunks))), n)   # a rank that holds a chunk
    patterns, budgets = [], []
    while len(patterns) < PER_BATCH:
        k = d.below(4)
        n = d.pick([m for m in PATTERN_LENS if m > k])
        text = d.pick(chunks)
        if len(text) < n:
            p = d.symbols(alphabet, n)
        else:
            at = d.below(len(text) - n + 1)
            p = bytes(d.pick(alphabet) if b == 0x0A else b for b in text[at:at + n])
        a = bytearray(p)
        for _ in range(d.below(k + 2)):             # 0 .. k + 1 substitutions (two may fall on one position)
            i = d.below(n)
            a[i] = d.pick([s for s in alphabet if s != a[i]])
        patterns.append(bytes(a))
        budgets.append(k)
    return Case(seed, alphabet, entries, chunks, limit, closed, setup, shard, patterns, budgets)
