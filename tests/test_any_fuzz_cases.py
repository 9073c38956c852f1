"""The generator of tests/any_fuzz_cases.py and the reference of tests/any_ref.py, judged without a device: the cases are
a function of the seed, well formed, and -- by the reference alone -- a mixture in which tests/test_any_fuzz_gpu.py cannot
pass on trivial inputs, without deduplicating anything or without folding anything.  What the issue asks of the committed
seeds is asserted HERE, not left to chance on the device."""
import pytest

from tests import any_ref
from tests.any_fuzz_cases import ALPHABETS, LETTERS, PER_BATCH, SEEDS, SETUPS, make_case
from tests.any_ref import AnyIcaseRef, AnyRef
from tests.search_fuzz_cases import LENGTHS


@pytest.fixture(scope='module')
def cases():
    return [make_case(s) for s in SEEDS]


def test_cases_are_a_function_of_the_seed(cases):
    assert [make_case(s) for s in SEEDS] == cases
    assert len({tuple(c.chunks) for c in cases}) == len(cases)


def test_cases_are_well_formed(cases):
    for c in cases:
        assert 1 <= len(c.chunks) and sum(len(t) for t in c.chunks) <= 65536
        text = b''.join(c.chunks) + (b'' if c.closed else b'\n')
        assert text == b''.join(e + b'\n' for e in c.entries)
        assert all(b'\n' not in e and len(e) in LENGTHS and set(e) <= set(c.alphabet) for e in c.entries) and (c.closed or c.entries[-1])
        assert c.closed or c.setup == 'device'
        assert c.shard is None or (c.setup == 'shard' and c.shard[0] < len(c.chunks))
        assert len(c.sets) == PER_BATCH and c.letters in LETTERS
        assert c.switches == ({} if c.letters is None else {'PSS_ICASE_SEED_LETTERS': c.letters})
        for alts in c.sets:                             # no set is refused: no case is skipped on the device
            assert 1 <= len(alts) <= 7 and all(alts)
            assert len(any_ref.normalise(alts, False)) <= any_ref.MAX_ALTS and len(any_ref.normalise(alts, True)) <= any_ref.MAX_ALTS_ICASE
    # every set-up of open_case is drawn, every alphabet, every letters setting; some last entry is unterminated
    assert {c.setup for c in cases} == set(SETUPS) == {'file', 'devices', 'shard', 'host', 'sa', 'device'}
    assert {c.alphabet for c in cases} == set(ALPHABETS) and {c.letters for c in cases} == set(LETTERS)
    assert {len(c.chunks) for c in cases} >= {1, 2, 3} and any(not c.closed for c in cases)


def overlapping(entries, alts):
    """Does some entry hold two alternatives one across the other's end -- neither apart nor one inside the other?"""
    for e in entries:
        for a in alts:
            for b in alts:
                at = e.find(a)
                while a != b and at >= 0:
                    for bt in range(at + 1, at + len(a)):
                        if e.startswith(b, bt) and bt + len(b) > at + len(a):
                            return True
                    at = e.find(a, at + 1)
    return False


def test_mixture(cases):
    """Over the committed seeds, for the exact form and under fold: at least a third of the sets have an entry that holds two
    distinct alternatives of the normalised set; some case has an overlapping pair; some has a match flush with a chunk's
    first byte and one flush with its last; some has equal seeds under fold; the normalisation drops something somewhere;
    the fold answer is strictly larger than the exact one in a quarter of the sets; half of the answers are neither empty
    nor every entry."""
    for icase, cls in ((False, AnyRef), (True, AnyIcaseRef)):
        sets = two = overlap = at_start = at_end = dropped = void = partial = 0
        for c in cases:
            ref = cls(c.chunks)
            n = sum(len(t) for t in ref._true)
            for alts in c.sets:
                norm = any_ref.normalise(alts, icase)
                held = ref.holding(norm)
                sets += 1
                two += any(len(h) >= 2 for h in held)
                dropped += len(norm) < len(alts)
                void += any(b'\n' in a for a in alts)
                partial += 0 < ref.search_any_ids(alts).size < n
                entries = [e for per in ref._entries() for e in per]
                overlap += overlapping(entries, norm)
                for per in ref._entries():
                    at_start += bool(per) and any(per[0].startswith(a) for a in norm)
                    at_end += bool(per) and any(per[-1].endswith(a) for a in norm)
        assert sets == len(SEEDS) * PER_BATCH
        assert 3 * two >= sets and overlap >= 1 and at_start >= 1 and at_end >= 1 and dropped >= 5 and void >= 1 and 2 * partial >= sets, \
            (icase, sets, two, overlap, at_start, at_end, dropped, void, partial)
    more = shared = 0
    for c in cases:
        exact, fold = AnyRef(c.chunks), AnyIcaseRef(c.chunks)
        for alts in c.sets:
            a, b = exact.search_any_ids(alts).tolist(), fold.search_any_ids(alts).tolist()
            assert set(a) <= set(b)
            more += len(b) > len(a)
            asked = any_ref.alternatives(alts, True, any_ref.LETTERS if c.letters is None else c.letters)
            shared += len({(pos, seed) for _, pos, seed in asked}) < len(asked) or len({seed for _, _, seed in asked}) < len(asked)
    assert 4 * more >= len(SEEDS) * PER_BATCH and shared >= 1, (more, shared)


def test_the_reference_states_one_order_per_answer(cases):
    """ordered_ids is a permutation of search_any_ids, whatever was given: duplicates, superstrings and newlines change
    neither the answer nor its order."""
    for c in cases[::3]:
        for icase, cls in ((False, AnyRef), (True, AnyIcaseRef)):
            ref = cls(c.chunks)
            ref.letters = any_ref.LETTERS if c.letters is None else c.letters
            for alts in c.sets:
                want, ordered = ref.search_any_ids(alts).tolist(), ref.ordered_ids(alts).tolist()
                assert sorted(ordered) == want and len(set(ordered)) == len(ordered)
                assert ref.ordered_ids(any_ref.normalise(alts, icase)).tolist() == ordered or not any_ref.normalise(alts, icase)
            assert ref.hits(c.sets) >= sum(ref.search_any_ids(alts).size for alts in c.sets)
