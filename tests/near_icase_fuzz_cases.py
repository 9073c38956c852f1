"""Seeded cases for the differential fuzz of the search within k mismatches / k edits under ASCII case folding: inputs
that nobody designed, for the brute-force references of tests/near_icase_ref.py to judge.

make_case(seed) follows tests/near_fuzz_cases.py and tests/edit_fuzz_cases.py -- the same _Draw, entry lengths and bodies,
chunk counts and setups, the same Case -- with three differences: the alphabets hold letters in BOTH CASES beside a digit,
the bytes one below the letters (`@`, '`'), 0x00 and bytes >= 0x80 (0xC1 / 0xE1 differ in the bit that folds `A` to `a`
and do not fold); a pattern, cut from the CHUNK TEXT (a newline inside the cut replaced by a symbol), gets the case of each
of its letters DRAWN ANEW; and then 0 .. k + 1 random edits at drawn positions -- a symbol inserted, a byte deleted (while
the pattern stays longer than its budget) or a byte substituted.  One batch serves both kinds.  CPU only;
tests/test_near_icase_fuzz_cases.py judges the generator and the references with it, tests/test_near_icase_fuzz_gpu.py runs
the engine on it."""
from tests.near_fuzz_cases import PATTERN_LENS, SETUPS, Case
from tests.search_fuzz_cases import _Draw, _entries, chunk_texts

__all__ = ['ALPHABETS', 'PATTERN_LENS', 'PER_BATCH', 'SEEDS', 'SETUPS', 'Case', 'make_case']

SEEDS = range(20)
PER_BATCH = 12
ALPHABETS = (b'aAbB', b'abcABC1', b'abcdefghABCDEFGH@`', b'\x00aA\xc1\xe1')


def make_case(seed: int) -> Case:
    d = _Draw(1900 + seed)
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
        a = bytearray(b ^ 0x20 if 0x61 <= (b | 0x20) <= 0x7a and d.chance(0.5) else b for b in p)      # the case of every letter anew
        for _ in range(d.below(k + 2)):             # 0 .. k + 1 edits
            op = d.below(3)
            if op == 0:
                a.insert(d.below(len(a) + 1), d.pick(alphabet))
            elif op == 1 and len(a) > k + 1:
                del a[d.below(len(a))]
            else:
                i = d.below(len(a))
                a[i] = d.pick([s for s in alphabet if s != a[i]])
        patterns.append(bytes(a))
        budgets.append(k)
    return Case(seed, alphabet, entries, chunks, limit, closed, setup, shard, patterns, budgets)
