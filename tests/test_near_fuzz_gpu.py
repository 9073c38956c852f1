"""Differential fuzz of the search within k mismatches: every seeded case of tests/near_fuzz_cases.py on the engine, the
whole batch through the check() of tests/search_harness.py -- ids, counts, order, text, hits, route and statistics against
the brute-force reference.  Per seed the index is written (or the chunks are handed over on the device, the only way to a
text without a closing newline) and the reader is opened as drawn: the file as written or split by max_chunk_len,
devices=[0, 0, 0] (whose merge is part-major: the order is not compared), one shard, the suffix arrays on the host tier.
tests/test_near_fuzz_cases.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

from tests.near_fuzz_cases import SEEDS, make_case
from tests.near_ref import NearRef
from tests.search_harness import NEAR, check, open_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, (ref,) = open_case(case, tmp_path, search_env, [NearRef], 'near')
    try:
        got = check(NEAR, r, ref, (case.patterns, case.budgets), order=case.setup != 'devices')
        assert got.counts.size == len(case.patterns)
        again = r.search_near_ids_batch(case.patterns, case.budgets)           # no state is left behind
        assert np.array_equal(again.ids, got.ids) and np.array_equal(again.counts, got.counts)
    finally:
        r.close()
