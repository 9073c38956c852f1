"""Differential fuzz of every entry-level search kind on the seeded cases of tests/search_fuzz_cases.py: inputs nobody
designed, judged by the brute-force references through the check() functions of the five kinds' own test files -- ids
against the reference, no id twice, the count call, the packed text against entries_by_id_packed, the route bits, the
stats, and for the case-insensitive search the exact order (except over several parts of one device, whose merge is
part-major).

Per seed: the index is written (or the chunks are handed over on the device, the only way to a text without a closing
newline), the drawn switches are set, the reader is opened as drawn -- the file as written or split by max_chunk_len,
devices=[0, 0, 0], one shard, the suffix arrays on the host tier, order='sa' -- and six batches run: entry ids, anchored
with an anchor per pattern, anchored under one anchor word, all-terms, wildcard, case-insensitive.  One of them then
runs once more and must return the identical ids: no kind leaves state behind for another.

run_case() is also what the time-boxed campaign of tests/tools/fuzz_search.py runs on fresh seeds."""
import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests import search_fuzz_cases as F
from tests.all_terms_ref import AllTermsRef
from tests.anchored_ref import AnchoredRef
from tests.entry_id_ref import IdRef
from tests.glob_ref import GlobRef
from tests.icase_ref import IcaseRef
from tests.test_all_terms_gpu import check as check_all_terms
from tests.test_anchored_gpu import check as check_anchored
from tests.test_entry_ids_gpu import check as check_ids
from tests.test_glob_gpu import check as check_glob
from tests.test_glob_gpu import device_reader, make_index
from tests.test_icase_gpu import check as check_icase

pytestmark = pytest.mark.gpu

BATCHES = ('ids', 'anchored', 'anchored_word', 'all_terms', 'glob', 'icase')
REFS = {'ids': IdRef, 'anchored': AnchoredRef, 'anchored_word': AnchoredRef, 'all_terms': AllTermsRef, 'glob': GlobRef, 'icase': IcaseRef}


def open_case(case, tmp_path, set_env):
    """(reader, {batch: reference}) of a case, the switches set."""
    set_env(**case.switches)
    if case.setup == 'device':
        return device_reader(case.chunks), {b: REFS[b](case.chunks) for b in BATCHES}
    assert case.closed
    p = make_index(tmp_path, 'fuzz%d' % case.seed, b''.join(case.chunks), case.max_chunk_len)
    keep = (lambda c: True) if case.shard is None else (lambda c: c % case.shard[1] == case.shard[0])
    refs = {b: REFS[b].from_index(p, keep=keep) for b in BATCHES}
    held = [c for c in range(len(case.chunks)) if keep(c)]
    for ref in refs.values():           # the Writer cut the file where the generator said it would
        assert [ch.index for ch in ref.chunks] == held and [ch.text for ch in ref.chunks] == [case.chunks[c] for c in held]
    if case.setup == 'devices':
        r = pysubstringsearch.Reader(p, devices=[0, 0, 0])
    elif case.setup == 'shard':
        r = pysubstringsearch.Reader(p, shard=case.shard)
    elif case.setup == 'sa':
        r = pysubstringsearch.Reader(p, order='sa')
    elif case.setup == 'host':          # one suffix array too many for the budget: it stays in pinned host memory
        probe = pysubstringsearch.Reader(p)
        hbm = probe.residency['hbm_bytes']
        probe.close()
        set_env(PSS_READER_HBM_BUDGET=hbm - 1, PSS_READER_AUTO_RESIDENCY=0)
        r = pysubstringsearch.Reader(p)
        assert r.residency['host_chunks'] >= 1
    else:
        r = pysubstringsearch.Reader(p)
    return r, refs


def run_batch(case, r, refs, batch):
    interval = None if case.interval is None else _ffi.ROUTES[case.interval]
    ref = refs[batch]
    if batch == 'ids':
        return check_ids(r, ref, case.ids)
    if batch == 'anchored':
        return check_anchored(r, ref, [p for p, _ in case.anchored], [k for _, k in case.anchored], interval=interval)
    if batch == 'anchored_word':
        return check_anchored(r, ref, *case.anchored_word, interval=interval)
    if batch == 'all_terms':
        return check_all_terms(r, ref, case.all_terms, interval=interval)
    if batch == 'glob':
        return check_glob(r, ref, [g for _, _, g in case.glob], interval=interval)
    return check_icase(r, ref, case.icase, order=case.setup != 'devices', interval=interval)


def run_case(case, tmp_path, set_env):
    r, refs = open_case(case, tmp_path, set_env)
    try:
        got = {b: run_batch(case, r, refs, b) for b in BATCHES}
        again = BATCHES[case.seed % len(BATCHES)]
        res = run_batch(case, r, refs, again)
        assert np.array_equal(res.ids, got[again].ids) and np.array_equal(res.counts, got[again].counts), again
        return got
    finally:
        r.close()


@pytest.mark.parametrize('seed', F.SEEDS)
def test_fuzz_every_kind(tmp_path, search_env, seed):
    run_case(F.make_case(seed), tmp_path, search_env)
