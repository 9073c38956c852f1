"""The generator of tests/near_icase_fuzz_cases.py and the references of tests/near_icase_ref.py, judged without a device:
the cases are a function of the seed, well formed, and -- by the references alone -- a mixture in which
tests/test_near_icase_fuzz_gpu.py cannot pass on trivial inputs or without folding anything."""
import pytest

from tests.edit_ref import EditRef
from tests.near_icase_fuzz_cases import ALPHABETS, PER_BATCH, SEEDS, SETUPS, make_case
from tests.near_icase_ref import CAP, LETTERS, EditIcaseRef, NearIcaseRef, is_letter
from tests.near_ref import NearRef, pieces
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
    assert all(any(is_letter(b) and is_letter(b ^ 0x20) and b ^ 0x20 in c.alphabet for b in c.alphabet) for c in cases)
    assert any(0 in c.alphabet and 0xc1 in c.alphabet and 0xe1 in c.alphabet for c in cases)


def test_mixture(cases):
    """Over the committed seeds: in at least a quarter of the rows the fold answer is strictly larger than the exact-case
    answer (for mismatches, and for edits too); in at least a quarter the edits answer is strictly larger than the mismatch
    answer; at least one half of the rows have an answer that is neither empty nor every entry; at least one row has a
    piece with more letters than the cap of its budget.  The relations of the contract hold in every row."""
    rows = fold_more = fold_more_edit = edit_more = partial = over_cap = 0
    for c in cases:
        near, edit, xnear, xedit = NearIcaseRef(c.chunks), EditIcaseRef(c.chunks), NearRef(c.chunks), EditRef(c.chunks)
        n = sum(len(t) for t in xnear._true)
        for p, k in zip(c.patterns, c.budgets):
            ham, lev = near.search_near_ids(p, k).tolist(), edit.search_edit_ids(p, k).tolist()
            xham, xlev = xnear.search_near_ids(p, k).tolist(), xedit.search_edit_ids(p, k).tolist()
            assert set(xham) <= set(ham) <= set(lev) and set(xlev) <= set(lev), (c.seed, p, k)
            if k == 0:
                assert ham == lev
            rows += 1
            fold_more += len(ham) > len(xham)
            fold_more_edit += len(lev) > len(xlev)
            edit_more += len(lev) > len(ham)
            partial += 0 < len(lev) < n
            over_cap += any(sum(map(is_letter, piece)) > min(LETTERS, CAP[k]) for _, piece in pieces(p, k))
    assert rows == len(SEEDS) * PER_BATCH
    assert 4 * fold_more >= rows and 4 * fold_more_edit >= rows and 4 * edit_more >= rows and 2 * partial >= rows and over_cap >= 1, \
        (rows, fold_more, fold_more_edit, edit_more, partial, over_cap)
