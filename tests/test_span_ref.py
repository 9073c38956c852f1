"""The brute-force reference of the match spans (tests/span_ref.py) judged without a GPU: its decision and its distance
against the Sellers scan of tests/edit_ref.py and the window count of tests/near_ref.py, its fast form against its naive
form, a few rows whose answer is obvious, and the MIXTURE of the seeded cases the GPU fuzz runs
(tests/test_span_fuzz_gpu.py): enough rows of every kind that a kernel which never ties, or never leaves its first step,
cannot pass there."""
import numpy as np

from tests.edit_ref import sellers
from tests.near_icase_fuzz_cases import SEEDS, make_case
from tests.near_ref import window_mismatches
from tests.span_ref import NONE, SpanRef, candidates, fold, lev, span, span_naive

ALPHABETS = (b'ab', b'aAbB', b'abc', b'\x00aA\xc1\xe1')


def _random_cases(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        alpha = ALPHABETS[int(rng.integers(0, len(ALPHABETS)))]
        k = int(rng.integers(0, 4))
        e = bytes(alpha[int(i)] for i in rng.integers(0, len(alpha), int(rng.integers(0, 14))))
        p = bytes(alpha[int(i)] for i in rng.integers(0, len(alpha), int(rng.integers(k + 1, k + 7))))
        yield e, p, k, bool(rng.integers(0, 2))


def test_decision_and_distance_are_sellers_and_the_window_count():
    matched = 0
    for e, p, k, icase in _random_cases(1000, 20):
        fe, fp = (fold(e), fold(p)) if icase else (e, p)
        got = span(e, p, k, True, icase)
        best = sellers(fe, fp)
        assert (got[2] >= 0) == (best <= k), (e, p, k, icase, got, best)
        if got[2] >= 0:
            matched += 1
            assert got[2] == best and lev(fe[got[0]:got[0] + got[1]], fp) == best and got[1] >= 1
        else:
            assert got == NONE
        got = span(e, p, k, False, icase)
        miss = window_mismatches(fe, fp)
        near = bool((miss <= k).any())
        assert (got[2] >= 0) == near, (e, p, k, icase, got)
        if near:
            assert got[1] == len(p) and got[2] == int(miss.min()) and got[0] == int(np.flatnonzero(miss == miss.min())[0])
    assert matched > 200


def test_fast_form_is_the_naive_form():
    for e, p, k, icase in _random_cases(400, 21):
        for edits in (False, True):
            assert span(e, p, k, edits, icase) == span_naive(e, p, k, edits, icase), (e, p, k, edits, icase)


def test_obvious_rows():
    assert span(b'passw0rd password', b'password', 1) == (9, 8, 0)                   # closest, not leftmost
    assert span(b'passw0rd password', b'password', 1, True) == (9, 8, 0)
    assert span(b'passw0rd passw1rd', b'password', 1) == (0, 8, 1)                    # then leftmost
    assert span(b'zbcd', b'abcd', 1, True) == (0, 4, 1)                               # then longest: `zbcd`, not `bcd`
    assert span(b'abxc', b'abc', 1, True) == (0, 4, 1)                                # `abxc`, not `ab`
    assert span(b'abc', b'abc', 2, True) == (0, 3, 0)
    assert span(b'xxPASSWORDxx', b'password', 0) == NONE
    assert span(b'xxPASSWORDxx', b'password', 0, icase=True) == (2, 8, 0)
    assert span(b'xxPaSSw0RDxx', b'pAssword', 1, True, True) == (2, 8, 1)
    assert span(b'\xc9', b'\xe9', 0, icase=True) == NONE and span(b'@[', b'`{', 1, icase=True) == NONE
    assert span(b'', b'a', 0) == NONE and span(b'', b'ab', 1, True) == NONE
    assert span(b'ab', b'abc', 0) == NONE and span(b'ab', b'abc', 1, True) == (0, 2, 1)
    assert span(b'a\nb'.replace(b'\n', b''), b'a\nb', 1) == NONE                      # a pattern with a newline
    assert span(b'b', b'abcd', 3, True) == (0, 1, 3)                                  # the shortest candidate: one byte


def test_mixture_of_the_seeded_cases():
    """Every entry of every seeded case against every pattern of the case, with the pattern's drawn budget, in the four
    combinations of edits x icase."""
    rows = none = other_start = other_length = left_of_winner = late = other_len_than_p = 0
    by_distance = {(edits, d): 0 for edits in (False, True) for d in range(4)}
    for seed in SEEDS:
        case = make_case(seed)
        ref = SpanRef(case.chunks)
        entries = [ref.true_entry(i) for i in ref.all_ids().tolist()]
        for edits in (False, True):
            for icase in (False, True):
                for p, k in zip(case.patterns, case.budgets):
                    for e in entries:
                        c = candidates(e, p, k, edits, icase)
                        rows += 1
                        if not len(c):
                            none += 1
                            continue
                        d, s, l = (int(x) for x in c[0])
                        by_distance[edits, d] += 1
                        same = c[c[:, 0] == d]
                        other_start += bool((same[:, 1] != s).any())
                        other_length += bool(((same[:, 1] == s) & (same[:, 2] != l)).any())
                        left_of_winner += bool((c[:, 1] < s).any())
                        late += s >= 64
                        other_len_than_p += l != len(p)
    print(dict(rows=rows, none=none, by_distance=by_distance, other_start=other_start, other_length=other_length,
               left_of_winner=left_of_winner, late=late, other_len_than_p=other_len_than_p))
    assert rows > 30000
    for what in (none, other_start, other_length, left_of_winner, late, other_len_than_p, *by_distance.values()):
        assert what >= 100
