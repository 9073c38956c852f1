"""Seeded cases for the differential fuzz of the any-of search: inputs that nobody designed, for the brute force of
tests/any_ref.py to judge.

make_case(seed) follows tests/near_icase_fuzz_cases.py -- the same _Draw, entry lengths and bodies, chunk counts, the same
alphabets with letters in both cases -- and draws every set-up of tests/search_harness.open_case (the six of
tests/search_fuzz_cases.py), the PSS_ICASE_SEED_LETTERS to set, and PER_BATCH sets of 1 .. 7 alternatives:
  * most alternatives are cut from the CHUNK TEXT (a newline inside the cut replaced by a symbol), several of one set from
    one entry, so that an entry holds two of them; in half of the sets the case of each letter is drawn anew, so that the
    fold has work;
  * an OVERLAPPING pair: two cuts of one stretch, one byte apart;
  * a cut flush with a chunk's first byte and one flush with its last (the closing newline apart);
  * lengths on both sides of the 8-byte register compare and a long one; random symbols; a duplicate, a superstring of
    another alternative and one that holds a newline -- what the normalisation drops;
  * now and then two alternatives that differ in their first byte alone: under fold, at few seed letters, they share a seed.
One batch serves both forms.  CPU only; tests/test_any_fuzz_cases.py judges the generator and the reference with it,
tests/test_any_fuzz_gpu.py runs the engine on it."""
import typing

from tests.near_icase_fuzz_cases import ALPHABETS
from tests.search_fuzz_cases import SETUPS, _Draw, _entries, chunk_texts

__all__ = ['ALPHABETS', 'ALT_LENS', 'LETTERS', 'PER_BATCH', 'SEEDS', 'SETUPS', 'Case', 'make_case']

SEEDS = range(24)
PER_BATCH = 10
ALT_LENS = (1, 2, 2, 3, 4, 5, 7, 8, 9, 12, 17, 40)
LETTERS = (None, 1, 6, 3)


class Case(typing.NamedTuple):
    seed: int
    alphabet: bytes
    entries: typing.List[bytes]
    chunks: typing.List[bytes]                  # the chunk texts: the entries with their newlines, in order
    max_chunk_len: typing.Optional[int]         # the Writer's argument that cuts the file into `chunks`
    closed: bool                                # False: the last chunk has no closing newline (setup == 'device')
    setup: str                                  # one of SETUPS
    shard: typing.Optional[typing.Tuple[int, int]]
    letters: typing.Optional[int]               # PSS_ICASE_SEED_LETTERS, or None for the default
    sets: typing.List[typing.List[bytes]]

    @property
    def switches(self) -> typing.Dict[str, int]:
        return {} if self.letters is None else {'PSS_ICASE_SEED_LETTERS': self.letters}


def make_case(seed: int) -> Case:
    d = _Draw(2200 + seed)
    alphabet = ALPHABETS[seed % len(ALPHABETS)]
    entries = _entries(d, alphabet, d.pick((3, 40, 120)))
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

    def clean(b: bytes) -> bytes:
        return bytes(d.pick(alphabet) if x == 0x0A else x for x in b)

    def recase(b: bytes) -> bytes:
        return bytes(x ^ 0x20 if 0x61 <= (x | 0x20) <= 0x7a and d.chance(0.4) else x for x in b)

    def cut(text: bytes, n: int, at: typing.Optional[int] = None) -> bytes:
        if len(text) < n:
            return d.symbols(alphabet, n)
        at = d.below(len(text) - n + 1) if at is None else at
        return clean(text[at:at + n])

    filled = [e for e in entries if e] or [d.symbols(alphabet, 5)]
    sets = []
    while len(sets) < PER_BATCH:
        alts, roll = [], d.below(10)
        e = d.pick(filled)
        for _ in range(d.between(2, 4)):            # several of one entry: it holds two of them
            alts.append(cut(e, min(len(e), d.pick(ALT_LENS))))
        if roll == 0:                               # an overlapping pair: two cuts of one stretch, one byte apart
            long_ = [x for x in filled if len(x) >= 6]
            if long_:
                x = d.pick(long_)
                n = d.between(3, min(9, len(x) - 1))
                at = d.below(len(x) - n)
                alts += [x[at:at + n], x[at + 1:at + n + 1]]
        elif roll == 1:                             # flush with a chunk's first byte and with its last
            text = d.pick(chunks)
            body = text[:-1] if text.endswith(b'\n') else text
            n = d.pick((1, 2, 5, 9))
            alts += [cut(body, n, 0), cut(body, n, max(0, len(body) - n))]
        elif roll == 2:                             # from anywhere in the text, entry borders included
            alts += [cut(d.pick(chunks), d.pick(ALT_LENS)) for _ in range(d.between(1, 3))]
        elif roll == 3:                             # what the normalisation drops
            a = d.pick(alts)
            alts += [a, d.symbols(alphabet, 1) + a + d.symbols(alphabet, 2), a[:1] + b'\n' + a]
        elif roll == 4:                             # two that differ in the first byte alone
            a = d.pick(alts)
            alts.append(bytes([d.pick([s for s in alphabet if s != a[0]])]) + a[1:])
        elif roll == 5:
            alts += [d.symbols(alphabet, d.pick(ALT_LENS)) for _ in range(d.between(1, 3))]
        anew = d.chance(0.5)                        # (half of the sets as they stand in the text: the exact form finds them too)
        alts = [recase(a) if anew else a for a in alts if a]
        for i in range(len(alts) - 1, 0, -1):       # (a shuffle out of the draws that keep their meaning across Python versions)
            j = d.below(i + 1)
            alts[i], alts[j] = alts[j], alts[i]
        if alts:
            sets.append(alts[:7])
    return Case(seed, alphabet, entries, chunks, limit, closed, setup, shard, LETTERS[(seed // 3) % len(LETTERS)], sets)
