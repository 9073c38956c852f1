"""The generator of tests/edit_fuzz_cases.py and the reference of tests/edit_ref.py, judged without a device: the cases are
a function of the seed, well formed, and -- by the references alone -- a mixture in which tests/test_edit_fuzz_gpu.py
cannot pass on trivial inputs."""
import pytest

from tests.edit_fuzz_cases import ALPHABETS, PER_BATCH, SEEDS, SETUPS, make_case
from tests.edit_ref import EditRef
from tests.near_ref import NearRef
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


def test_mixture(cases):
    """Over the committed seeds, of the (pattern, k >= 1) pairs at least one quarter have an edit answer strictly larger
    than the Hamming answer at the same k -- insertions and deletions decide something -- and at least one half have an answer
    that is neither empty nor every entry.  Every edit answer contains the Hamming answer, and k = 0 is the same answer."""
    pairs = larger = partial = 0
    for c in cases:
        ref, near = EditRef(c.chunks), NearRef(c.chunks)
        n = sum(len(t) for t in ref._true)
        for p, k in zip(c.patterns, c.budgets):
            ids, ham = ref.search_edit_ids(p, k).tolist(), near.search_near_ids(p, k).tolist()
            assert set(ham) <= set(ids), (c.seed, p, k)
            if k == 0:
                assert ids == ham
                continue
            pairs += 1
            larger += len(ids) > len(ham)
            partial += 0 < len(ids) < n
    assert pairs >= len(SEEDS) * PER_BATCH // 2
    assert 4 * larger >= pairs and 2 * partial >= pairs, (pairs, larger, partial)
