"""The seeded cases of tests/regex_fuzz_cases.py on the GPU: every case's reader opened as drawn (open_case of
tests/search_harness.py), its two batches of regular expressions through check() against the brute-force reference of
tests/regex_ref.py, exact and under icase=True."""
import pytest

from tests import search_harness as H
from tests.regex_fuzz_cases import SEEDS, make_regex_case
from tests.regex_ref import REGEX, REGEX_ICASE, RegexRef

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', SEEDS)
def test_case(seed, tmp_path, search_env):
    case = make_regex_case(seed)
    base = case.base
    r, (ref,) = H.open_case(base, tmp_path, search_env, [RegexRef], 'regex')
    interval = None if base.interval is None else H.R[base.interval]
    try:
        order = base.setup != 'devices'
        first = H.check(REGEX, r, ref, case.regex, order=order, interval=interval)
        H.check(REGEX_ICASE, r, ref, case.regex_icase, order=order, interval=interval)
        again = H.check(REGEX, r, ref, case.regex, order=order, interval=interval)
        assert (again.ids == first.ids).all() and (again.counts == first.counts).all()
    finally:
        r.close()
        search_env(**{k: None for k in list(base.switches) + ['PSS_READER_HBM_BUDGET', 'PSS_READER_AUTO_RESIDENCY']})
