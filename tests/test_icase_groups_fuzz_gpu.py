"""Differential fuzz of the case-insensitive all-terms and wildcard search: every seeded case of
tests/icase_groups_fuzz_cases.py on the engine, every group and every pattern through the check() of
tests/search_harness.py -- ids, counts, order, text, route and statistics against the brute-force reference.
tests/test_icase_groups_fuzz_cases.py vouches for the mixture of the cases; no case is skipped here."""
import pytest

from tests.icase_groups_fuzz_cases import SEEDS, make_case
from tests.icase_groups_ref import IcaseGroupsRef
from tests.search_harness import ICASE_ALL, ICASE_GLOB, check, device_reader

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, search_env):
    case = make_case(seed)
    search_env(PSS_ICASE_SEED_LETTERS=case.letters)
    r, ref = device_reader(case.chunks), IcaseGroupsRef(case.chunks)
    try:
        got = check(ICASE_ALL, r, ref, case.groups)
        assert got.counts.size == len(case.groups)
        got = check(ICASE_GLOB, r, ref, case.globs)
        assert got.counts.size == len(case.globs)
    finally:
        r.close()
