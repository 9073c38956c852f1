"""Differential fuzz of the search within k edits: every seeded case of tests/edit_fuzz_cases.py on the engine, the whole
batch through the check() of tests/test_edit_gpu.py -- ids, counts, order, text, hits, route and statistics against the
brute-force reference.  The reader is opened as drawn, by the open_case of tests/test_near_fuzz_gpu.py with the edit
reference in it.  tests/test_edit_fuzz_cases.py vouches for the mixture of the cases; no case is skipped here."""
import numpy as np
import pytest

import pysubstringsearch
from tests.edit_fuzz_cases import SEEDS, make_case
from tests.edit_ref import EditRef
from tests.test_edit_gpu import check, device_reader, make_index

pytestmark = pytest.mark.gpu


def open_case(case, tmp_path, set_env):
    """(reader, reference) of a case."""
    if case.setup == 'device':
        return device_reader(case.chunks), EditRef(case.chunks)
    assert case.closed
    p = make_index(tmp_path, 'edit%d' % case.seed, b''.join(case.chunks), case.max_chunk_len)
    keep = (lambda c: True) if case.shard is None else (lambda c: c % case.shard[1] == case.shard[0])
    ref = EditRef.from_index(p, keep=keep)
    held = [c for c in range(len(case.chunks)) if keep(c)]          # the Writer cut the file where the generator said it would
    assert [ch.index for ch in ref.chunks] == held and [ch.text for ch in ref.chunks] == [case.chunks[c] for c in held]
    if case.setup == 'devices':
        return pysubstringsearch.Reader(p, devices=[0, 0, 0]), ref
    if case.setup == 'shard':
        return pysubstringsearch.Reader(p, shard=case.shard), ref
    if case.setup == 'host':            # one suffix array too many for the budget: it stays in pinned host memory
        probe = pysubstringsearch.Reader(p)
        hbm = probe.residency['hbm_bytes']
        probe.close()
        set_env(PSS_READER_HBM_BUDGET=hbm - 1, PSS_READER_AUTO_RESIDENCY=0)
        r = pysubstringsearch.Reader(p)
        assert r.residency['host_chunks'] >= 1
        return r, ref
    return pysubstringsearch.Reader(p), ref


@pytest.mark.parametrize('seed', list(SEEDS))
def test_fuzz(seed, tmp_path, search_env):
    case = make_case(seed)
    r, ref = open_case(case, tmp_path, search_env)
    try:
        got = check(r, ref, case.patterns, case.budgets, order=case.setup != 'devices')
        assert got.counts.size == len(case.patterns)
        again = r.search_near_ids_batch(case.patterns, case.budgets, edits=True)           # no state is left behind
        assert np.array_equal(again.ids, got.ids) and np.array_equal(again.counts, got.counts)
    finally:
        r.close()
