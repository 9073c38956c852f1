"""The generator of tests/icase_groups_fuzz_cases.py and the reference of tests/icase_groups_ref.py, judged without a
device: the cases are a function of the seed, well formed, and -- by the reference alone -- a mixture in which
tests/test_icase_groups_fuzz_gpu.py cannot pass vacuously."""
import pytest

from pysubstringsearch_amd import glob_parse
from tests.icase_groups_fuzz_cases import PER_BATCH, SEEDS, make_case
from tests.icase_groups_ref import IcaseGroupsRef


@pytest.fixture(scope='module')
def cases():
    return [make_case(s) for s in SEEDS]


def test_cases_are_a_function_of_the_seed(cases):
    assert [make_case(s) for s in SEEDS] == cases
    assert len({tuple(c.chunks) for c in cases}) == len(cases)


def test_cases_are_well_formed(cases):
    for c in cases:
        assert 1 <= len(c.chunks) <= 4 and sum(len(t) for t in c.chunks) <= 65536
        text = b''.join(c.chunks) + (b'' if c.closed else b'\n')
        assert text == b''.join(e + b'\n' for e in c.entries)
        assert all(b'\n' not in e for e in c.entries) and (c.closed or c.entries[-1])
        assert len(c.groups) == len(c.globs) == PER_BATCH
        for include, exclude in c.groups:
            assert include and all(include) and all(exclude)
        for g in c.globs:
            segs, anchors = glob_parse(g)
            assert segs and all(segs) and 0 <= anchors <= 3
    assert {len(c.chunks) for c in cases} >= {1, 2, 3} and {c.closed for c in cases} == {True, False}
    assert {c.letters for c in cases} == {None, 1, 3, 6}


def test_mixture(cases, search_env):
    """Over the committed seeds: >= 60 % of the groups and of the patterns have an answer, >= 10 % have none, >= 20 % have
    an exclusion that takes an entry away or an anchor, and in >= 20 % the driver of some chunk is not the first term."""
    for kind in ('all', 'glob'):
        total = hit = empty = narrowed = late = 0
        for c in cases:
            search_env(PSS_ICASE_SEED_LETTERS=c.letters)
            ref = IcaseGroupsRef(c.chunks)
            for q in (c.groups if kind == 'all' else c.globs):
                total += 1
                ids = ref.search_all_ids(q) if kind == 'all' else ref.search_glob_ids(q)
                hit += ids.size > 0
                empty += ids.size == 0
                if kind == 'all':
                    narrowed += bool(q[1]) and ref.search_all_ids((q[0], [])).size > ids.size
                else:
                    narrowed += glob_parse(q)[1] != 0
                late += any(d not in (0, None) for d in ref.drivers(kind, q))
                assert ref.ordered_ids(kind, q).size == ids.size
        assert total == len(SEEDS) * PER_BATCH
        assert hit >= 0.6 * total, (kind, hit, total)
        assert empty >= 0.1 * total, (kind, empty, total)
        assert narrowed >= 0.2 * total, (kind, narrowed, total)
        assert late >= 0.2 * total, (kind, late, total)
