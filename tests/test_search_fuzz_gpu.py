"""Differential fuzz of every entry-level search kind on the seeded cases of tests/search_fuzz_cases.py: inputs nobody
designed, judged by the brute-force references through the check() of tests/search_harness.py under each kind -- ids
against the reference, no id twice, the count call, the packed text against entries_by_id_packed, the route bits, the
stats, and for the case-insensitive search the exact order (except over several parts of one device, whose merge is
part-major).

Per seed: the index is written (or the chunks are handed over on the device, the only way to a text without a closing
newline), the drawn switches are set, the reader is opened as drawn -- the file as written or split by max_chunk_len,
devices=[0, 0, 0], one shard, the suffix arrays on the host tier, order='sa' -- and six batches run: entry ids, anchored
with an anchor per pattern, anchored under one anchor word, all-terms, wildcard, case-insensitive.  One of them then
runs once more and must return the identical ids: no kind leaves state behind for another.

run_case() of tests/search_harness.py is also what the time-boxed campaign of tests/tools/fuzz_search.py runs on fresh seeds."""
import pytest

from tests import search_fuzz_cases as F
from tests.search_harness import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', F.SEEDS)
def test_fuzz_every_kind(tmp_path, search_env, seed):
    run_case(F.make_case(seed), tmp_path, search_env)
