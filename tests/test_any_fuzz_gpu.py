"""Differential fuzz of the any-of search: every seeded case of tests/any_fuzz_cases.py on the engine, the whole batch
through the check() of tests/search_harness.py in exact bytes and under fold -- ids, counts, order, text, hits, route and
statistics against the brute force of tests/any_ref.py.  The reader is opened as drawn, by the open_case of
tests/search_harness.py.  tests/test_any_fuzz_cases.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

from tests import any_ref
from tests.any_fuzz_cases import SEEDS, make_case
from tests.any_ref import ANY, ANY_ICASE, AnyIcaseRef, AnyRef
from tests.search_harness import check, open_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, refs = open_case(case, tmp_path, search_env, [AnyRef, AnyIcaseRef], 'any')
    try:
        got = []
        for kind, ref in zip((ANY, ANY_ICASE), refs):
            ref.letters = any_ref.LETTERS if case.letters is None else case.letters
            got.append(check(kind, r, ref, case.sets, order=case.setup != 'devices'))
            assert got[-1].counts.size == len(case.sets)
        assert (got[0].counts <= got[1].counts).all()
        for res, icase in zip(got, (False, True)):                                    # no state is left behind
            again = r.search_any_ids_batch(case.sets, icase=icase)
            assert np.array_equal(again.ids, res.ids) and np.array_equal(again.counts, res.counts)
    finally:
        r.close()
