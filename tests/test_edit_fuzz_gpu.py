"""Differential fuzz of the search within k edits: every seeded case of tests/edit_fuzz_cases.py on the engine, the whole
batch through the check() of tests/search_harness.py -- ids, counts, order, text, hits, route and statistics against the
brute-force reference.  The reader is opened as drawn, by the open_case of tests/search_harness.py with the edit
reference in it.  tests/test_edit_fuzz_cases.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

from tests.edit_fuzz_cases import SEEDS, make_case
from tests.edit_ref import EditRef
from tests.search_harness import EDIT, check, open_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, (ref,) = open_case(case, tmp_path, search_env, [EditRef], 'edit')
    try:
        got = check(EDIT, r, ref, (case.patterns, case.budgets), order=case.setup != 'devices')
        assert got.counts.size == len(case.patterns)
        again = r.search_near_ids_batch(case.patterns, case.budgets, edits=True)           # no state is left behind
        assert np.array_equal(again.ids, got.ids) and np.array_equal(again.counts, got.counts)
    finally:
        r.close()
