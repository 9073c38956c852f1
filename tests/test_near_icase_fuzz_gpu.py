"""Differential fuzz of the search within k mismatches and within k edits under ASCII case folding: every seeded case of
tests/near_icase_fuzz_cases.py on the engine, the whole batch through the check() of tests/search_harness.py under both
kinds -- ids, counts, order, text, hits, route and statistics against the brute-force references.  The reader is opened as
drawn, by the open_case of tests/search_harness.py.  tests/test_near_icase_fuzz_cases.py vouches for the mixture of the
cases; no case is skipped here."""
import numpy as np
import pytest

from tests.near_icase_fuzz_cases import SEEDS, make_case
from tests.near_icase_ref import EditIcaseRef, NearIcaseRef
from tests.search_harness import _near, check, open_case

pytestmark = pytest.mark.gpu

NEAR = _near('near_icase', NearIcaseRef, lambda ref, p, k: ref.search_near_ids(p, k), icase=True)
EDIT = _near('edit_icase', EditIcaseRef, lambda ref, p, k: ref.search_edit_ids(p, k), edits=True, icase=True)


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, refs = open_case(case, tmp_path, search_env, [NearIcaseRef, EditIcaseRef], 'near_icase')
    try:
        got = []
        for kind, ref in zip((NEAR, EDIT), refs):
            got.append(check(kind, r, ref, (case.patterns, case.budgets), order=case.setup != 'devices'))
            assert got[-1].counts.size == len(case.patterns)
        for res, edits in zip(got, (False, True)):                                    # no state is left behind
            again = r.search_near_ids_batch(case.patterns, case.budgets, edits=edits, icase=True)
            assert np.array_equal(again.ids, res.ids) and np.array_equal(again.counts, res.counts)
    finally:
        r.close()
