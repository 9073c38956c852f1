"""Differential fuzz of the match spans: the seeded cases of tests/near_icase_fuzz_cases.py on the engine, the reader opened
as drawn by the open_case of tests/search_harness.py.  Per case and per combination of edits x icase, every id of the reader
against the case's 12 patterns in ONE match_spans_batch call equals the brute-force reference of tests/span_ref.py row for
row, and the ids with distance >= 0 are, per pattern, exactly the ids search_near_ids_batch returns for the same arguments.
tests/test_span_ref.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

from tests.near_icase_fuzz_cases import PER_BATCH, SEEDS, make_case
from tests.search_harness import open_case, per_row
from tests.span_ref import SpanRef

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, (ref,) = open_case(case, tmp_path, search_env, [SpanRef], 'span')
    try:
        ids = ref.all_ids()
        nq = len(case.patterns)
        assert nq == PER_BATCH and ids.size
        all_ids, counts = np.tile(ids, nq), [ids.size] * nq
        for edits in (False, True):
            for icase in (False, True):
                got = r.match_spans_batch(all_ids, counts, case.patterns, case.budgets, edits, icase=icase)
                want = ref.spans(all_ids, counts, case.patterns, case.budgets, edits, icase)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert not bad.size, (edits, icase, 'rows wrong', int(bad.size), 'first', int(bad[0]), ref.true_entry(all_ids[bad[0]])[:80],
                                      case.patterns[int(bad[0]) // ids.size], case.budgets[int(bad[0]) // ids.size],
                                      got[bad[0]].tolist(), want[bad[0]].tolist())
                found = r.search_near_ids_batch(case.patterns, case.budgets, edits=edits, icase=icase)
                for q, row in enumerate(per_row(found)):
                    mine = ids[got[q * ids.size:(q + 1) * ids.size, 2] >= 0]
                    assert np.array_equal(mine, np.sort(row)), (edits, icase, q, case.patterns[q], case.budgets[q])
                if not edits:
                    assert (got[got[:, 2] >= 0][:, 1] == np.repeat([len(p) for p in case.patterns], ids.size)[got[:, 2] >= 0]).all()
    finally:
        r.close()
