"""Differential fuzz of the wildcard search with byte classes: every seeded case of tests/glob_class_fuzz_cases.py on the
engine, the reader opened as the case drew it, every pattern through the check() of tests/search_harness.py -- ids,
counts, text, route and statistics against the brute-force reference of tests/glob_class_ref.py --, exact and under
fold.  Then the plain glob batch of the same corpus twice on the same reader, with identical ids: the class search leaves
no state behind.  tests/test_glob_class_host.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

from tests import search_harness as H
from tests.glob_class_fuzz_cases import SEEDS, make_case
from tests.glob_class_ref import GlobClassRef
from tests.glob_ref import GlobRef
from tests.test_glob_class_gpu import CLASS, CLASS_ICASE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, (ref, plain) = H.open_case(case, tmp_path, search_env, [GlobClassRef, GlobRef], 'globclass')
    interval = None if case.interval is None else H.R[case.interval]
    try:
        first = H.check(H.GLOB, r, plain, case.glob, interval=interval)
        got = H.check(CLASS, r, ref, case.patterns, interval=interval)
        assert got.counts.size == len(case.patterns)
        got = H.check(CLASS_ICASE, r, ref, case.patterns, interval=interval)
        assert got.counts.size == len(case.patterns)
        again = H.check(H.GLOB, r, plain, case.glob, interval=interval)
        assert np.array_equal(again.ids, first.ids) and np.array_equal(again.counts, first.counts)
    finally:
        r.close()
