"""The generator of tests/near_fuzz_cases.py and the reference of tests/near_ref.py, judged without a device: the cases are
a function of the seed, well formed, and -- by the reference alone -- a mixture in which tests/test_near_fuzz_gpu.py
cannot pass vacuously."""
import numpy as np
import pytest

from tests.near_fuzz_cases import ALPHABETS, PER_BATCH, SEEDS, SETUPS, make_case
from tests.near_ref import NearRef, near_starts, pieces, window_mismatches
from tests.search_fuzz_cases import LENGTHS


@pytest.fixture(scope='module')
def cases():
    return [make_case(s) for s in SEEDS]


def test_cases_are_a_function_of_the_seed(cases):
    assert [make_case(s) for s in SEEDS] == cases
    assert len({tuple(c.chunks) for c in cases}) == len(cases)


def test_cases_are_well_formed(cases):
    for c in cases:
        assert 1 <= len(c.chunks) and sum(len(t) for t in c.chunks) <= 65536
        text = b''.join(c.chunks) + (b'' if c.closed else b'\n')
        assert text == b''.join(e + b'\n' for e in c.entries)
        assert all(b'\n' not in e and len(e) in LENGTHS and set(e) <= set(c.alphabet) for e in c.entries) and (c.closed or c.entries[-1])
        assert c.closed or c.setup == 'device'
        assert c.shard is None or (c.setup == 'shard' and c.shard[0] < len(c.chunks))
        assert len(c.patterns) == len(c.budgets) == PER_BATCH
        for p, k in zip(c.patterns, c.budgets):
            assert 0 <= k <= 3 and len(p) > k and b'\n' not in p and set(p) <= set(c.alphabet)
    assert {c.setup for c in cases} == set(SETUPS) and {c.alphabet for c in cases} == set(ALPHABETS)
    assert {len(c.chunks) for c in cases} >= {1, 2, 3} and {c.closed for c in cases} == {True, False}
    assert {k for c in cases for k in c.budgets} == {0, 1, 2, 3}
    assert any(0 in c.alphabet and max(c.alphabet) >= 0x80 for c in cases)


def crosses_a_newline(chunks, p, k):
    """Does some window of a chunk text hold p within k mismatches AND a newline?  (No match, by the contract.)"""
    q = np.frombuffer(p, np.uint8)
    for t in chunks:
        if len(t) >= len(p):
            w = np.lib.stride_tricks.sliding_window_view(np.frombuffer(t, np.uint8), len(p))
            if (((w != q).sum(axis=1) <= k) & (w == 0x0A).any(axis=1)).any():
                return True
    return False


def test_mixture(cases):
    """Over the committed seeds, of the 480 (pattern, k) pairs at least one in ten -- 48 -- is of each kind the kernels can
    go wrong on: a nearest window at EXACTLY k mismatches (k > 0: one more and it is lost), a nearest window at k + 1
    (one fewer and it is found), a window within budget that reaches across a newline, a pattern with repeated pieces,
    an entry with two near matches (the dedupe has something to drop); and at least half have an answer, one in ten none.
    (The committed seeds hold 65, 79, 170, 58 and 240 of them, 348 with an answer.)"""
    total = at_k = at_k1 = across = repeated = twice = hit = empty = 0
    for c in cases:
        ref = NearRef(c.chunks)
        entries = [e for t in ref._true for e in t]
        for p, k in zip(c.patterns, c.budgets):
            total += 1
            fit = [e for e in entries if len(e) >= len(p)]
            nearest = min([int(window_mismatches(e, p).min()) for e in fit] or [99])
            ids = ref.search_near_ids(p, k)
            assert (ids.size > 0) == (nearest <= k) and ref.ordered_ids(p, k).size == ids.size
            hit += ids.size > 0
            empty += ids.size == 0
            at_k += k > 0 and nearest == k
            at_k1 += nearest == k + 1
            across += crosses_a_newline(c.chunks, p, k)
            repeated += len({piece for _, piece in pieces(p, k)}) <= k
            twice += any(near_starts(e, p, k).size >= 2 for e in fit)
    assert total == len(SEEDS) * PER_BATCH == 480
    assert hit >= total // 2 and empty >= total // 10, (hit, empty)
    for name, n in (('at k', at_k), ('at k + 1', at_k1), ('across a newline', across), ('repeated pieces', repeated), ('two near matches', twice)):
        assert n >= 48, (name, n)
