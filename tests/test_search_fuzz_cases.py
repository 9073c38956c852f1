"""The seeded case generator of tests/search_fuzz_cases.py and the five brute-force references that judge the engine on
its cases (tests/test_search_fuzz_gpu.py), on the CPU: no engine call.
  * the cases are a pure function of the seed, and the seed set's cases are pinned by a hash: the inputs on which the
    conditions below were established do not drift unnoticed;
  * the mixture, measured by the references alone: per kind, over the seed set, at least 40 % of the patterns have an
    answer, at least 10 % have none, and for at least 30 % the verify step has something to reject or to find; every
    alphabet, entry length, shape, set-up and switch is drawn; and the patterns that only a scan with the right
    leftmost / no-overlap / fold rules answers correctly are there;
  * the references agree with each other wherever two of them mean the same."""
import hashlib
import itertools

import numpy as np
import pytest

from pysubstringsearch_amd import glob_parse
from tests import search_fuzz_cases as F
from tests.all_terms_ref import AllTermsRef
from tests.anchored_ref import AnchoredRef
from tests.entry_id_ref import IdRef
from tests.glob_ref import END, START, GlobRef
from tests.icase_ref import IcaseRef

CASES_SHA256 = '03a0278044d2cbcda191fd81a84d7ae0075a88c169ad0bdd2f7d11ce4f556a2b'
KINDS = ('anchored', 'all_terms', 'glob', 'icase')


class Refs:
    def __init__(self, case):
        t = case.chunks
        self.ids, self.anchored, self.terms, self.glob, self.icase = IdRef(t), AnchoredRef(t), AllTermsRef(t), GlobRef(t), IcaseRef(t)
        self.entries = [e for ch in self.glob._true for e in ch]            # every entry with all its bytes, in id order
        self.all_ids = [(ch.index << 32) | line for ch, es in zip(self.glob.chunks, self.glob._true) for line in range(len(es))]


@pytest.fixture(scope='module')
def cases():
    return [F.make_case(s) for s in F.SEEDS]


@pytest.fixture(scope='module')
def judged(cases):
    return [(c, Refs(c)) for c in cases]


# ---- determinism ------------------------------------------------------------------------------------------------------

def test_cases_are_a_function_of_the_seed(cases):
    for c in cases:
        assert F.case_bytes(F.make_case(c.seed)) == F.case_bytes(c)
    assert F.case_bytes(cases[0]) != F.case_bytes(cases[1])
    h = hashlib.sha256()
    for c in cases:
        h.update(F.case_bytes(c))
    assert h.hexdigest() == CASES_SHA256


def test_cases_are_well_formed(cases):
    for c in cases:
        text = b''.join(e + b'\n' for e in c.entries)
        assert b''.join(c.chunks) == (text if c.closed else text[:-1]) and all(c.chunks)
        assert all(b'\n' not in e and b'\r' not in e and set(e) <= set(c.alphabet) for e in c.entries)
        assert all(len(e) in F.LENGTHS for e in c.entries)
        assert c.closed or (c.setup == 'device' and c.entries[-1])
        assert c.max_chunk_len is not None or len(c.chunks) == 1
        assert F.chunk_texts(c.entries, c.max_chunk_len)[:-1] == c.chunks[:-1]
        assert c.max_chunk_len is None or all(len(e) + 1 <= c.max_chunk_len for e in c.entries)
        assert (c.shard is not None) == (c.setup == 'shard') and (c.shard is None or c.shard[0] < min(c.shard[1], len(c.chunks)))
        flat = c.ids + [p for p, _ in c.anchored] + c.anchored_word[0] + c.icase
        flat += [t for inc, exc in c.all_terms for t in inc + exc] + [s for segs, _, _ in c.glob for s in segs]
        assert all(p and b'\n' not in p for p in flat)
        assert all(inc and len(inc) <= 5 and len(exc) <= 2 for inc, exc in c.all_terms)
        for segs, anchors, pattern in c.glob:
            assert glob_parse(pattern) == (segs, anchors) and 1 <= len(segs) <= 8
        for batch in (c.ids, c.anchored, c.anchored_word[0], c.all_terms, c.glob, c.icase):
            assert len(batch) == F.PER_BATCH


def test_everything_is_drawn(cases):
    assert {c.alphabet for c in cases} == set(F.ALPHABETS)
    assert {len(e) for c in cases for e in c.entries} == set(F.LENGTHS)
    assert {len(c.entries) for c in cases} == {1, 3, 40, 300}
    assert {c.setup for c in cases} == set(F.SETUPS)
    assert {min(len(c.chunks), 5) for c in cases} >= {1, 2, 5} and any(c.max_chunk_len for c in cases if c.setup != 'device')
    assert any(not c.closed for c in cases) and any(c.closed and c.setup == 'device' for c in cases)
    assert {c.interval for c in cases} == {None, 'INTERVAL_WAVE', 'INTERVAL_LANE'}
    drawn = {(k, v) for c in cases for k, v in c.switches.items()}
    assert {k for k, _ in drawn} == {'PSS_LANE_SEARCH_MIN', 'PSS_WAVE_SEARCH', 'PSS_NO_GROUP_SEARCH', 'PSS_NO_SEARCH_STAGE', 'PSS_NO_PINNED_RESULTS',
                                     'PSS_NO_MID_PIPELINE', 'PSS_SAMPLE_SHIFT', 'PSS_NO_KEY_SAMPLES', 'PSS_ICASE_SEED_LETTERS'}
    assert {v for k, v in drawn if k == 'PSS_LANE_SEARCH_MIN'} == {1, 100000}
    assert len({v for k, v in drawn if k == 'PSS_ICASE_SEED_LETTERS'}) >= 4 and any('PSS_ICASE_SEED_LETTERS' not in c.switches for c in cases)
    assert {w for c in cases for _, w in c.anchored} == {c.anchored_word[1] for c in cases} == set(F.KINDS)
    assert {a for c in cases for _, a, _ in c.glob} == {0, 1, 2, 3} and {len(s) for c in cases for s, _, _ in c.glob} >= {1, 2, 3, 4}


# ---- the mixture ------------------------------------------------------------------------------------------------------

def answers(case, refs, kind):
    """Per pattern of the kind's batch: (entries in the answer, has the verify step something to reject or to find?)."""
    out = []
    if kind == 'anchored':
        for p, k in case.anchored:
            n = refs.anchored.search_ids(p, k).size
            out.append((n, refs.ids.search_ids(p).size > n))         # more entries contain it than match it under its anchor
    elif kind == 'all_terms':
        for inc, exc in case.all_terms:
            n = refs.terms.search_all_ids((inc, exc)).size
            out.append((n, min(refs.terms.term_ids(t).size for t in inc) > n))       # the rarest include term is in more entries
    elif kind == 'glob':
        for segs, anchors, _ in case.glob:
            n = refs.glob.search_seq_ids(segs, anchors).size
            out.append((n, refs.terms.search_all_ids((segs, [])).size > n))          # order, overlap or an anchor decided
    else:
        for p in case.icase:
            n = refs.icase.search_icase_ids(p).size
            out.append((n, n > refs.ids.search_ids(p).size))                         # only the fold found them
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_mixture(judged, kind):
    got = [x for case, refs in judged for x in answers(case, refs, kind)]
    total = len(got)
    assert total == len(F.SEEDS) * F.PER_BATCH >= 960
    hit = sum(1 for a, _ in got if a > 0)
    work = sum(1 for _, w in got if w)
    print(f'{kind}: {total} patterns, {hit} with an answer, {total - hit} without, {work} with work for the verify step')
    assert hit >= 0.40 * total and total - hit >= 0.10 * total and work >= 0.30 * total


def overlapping_walk(e, segs, anchors):
    """Does e match if a segment may begin anywhere behind the START of the one before it?  The walk of the engine's
    verify step (END, then START, then left to right at the leftmost occurrence) with `from` advanced by one byte."""
    segs = list(segs)
    lo, lim = 0, len(e)
    if anchors == 3 and len(segs) == 1:
        return e == segs[0]
    if anchors & END:
        last = segs.pop()
        if len(last) > lim or e[lim - len(last):] != last:
            return False
        lim -= len(last)
    if anchors & START and segs:
        first = segs.pop(0)
        if len(first) > lim or e[:len(first)] != first:
            return False
        lo = len(first)
    for s in segs:
        at = e.find(s, lo, lim)
        if at < 0:
            return False
        lo = at + 1
    return True


def test_the_patterns_that_tell_the_rules_apart(judged):
    overlap = both_anchors = spellings = fold_edge = exclude = 0
    for case, refs in judged:
        for segs, anchors, _ in case.glob:
            want = set(refs.glob.search_seq_ids(segs, anchors).tolist())
            loose = {i for i, e in zip(refs.all_ids, refs.entries) if overlapping_walk(e, segs, anchors)}
            assert want <= loose
            overlap += loose != want
            both_anchors += anchors == 3 and len(segs) >= 2 and bool(want)
        by_id = dict(zip(refs.all_ids, refs.entries))
        for p in case.icase:
            low, found = p.lower(), refs.icase.search_icase_ids(p).tolist()
            for i in found:
                e, el = by_id[i], by_id[i].lower()
                at, seen = el.find(low), set()
                while at >= 0:
                    seen.add(e[at:at + len(p)])
                    at = el.find(low, at + 1)
                if len(seen) >= 2:
                    spellings += 1
                    break
            if not found:
                near = [p[:k] + bytes([x ^ 0x20]) + p[k + 1:] for k, x in enumerate(p) if x in b'@[`{' or x >= 0x80]
                fold_edge += any(refs.icase.search_icase_ids(q).size for q in near)
        for inc, exc in case.all_terms:
            exclude += refs.terms.search_all_ids((inc, [])).size > refs.terms.search_all_ids((inc, exc)).size
    print(f'overlap decides {overlap}, both anchors with 2+ segments {both_anchors}, two spellings in one entry {spellings}, '
          f'a miss one fold edge away from a hit {fold_edge}, an exclude term removes an entry {exclude}')
    assert overlap >= 1 and both_anchors >= 1 and spellings >= 1 and fold_edge >= 1 and exclude >= 1


# ---- the references judge each other ----------------------------------------------------------------------------------

def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))


def all_spellings(p):
    choices = [(bytes([b & ~0x20]), bytes([b | 0x20])) if F.is_letter(b) else (bytes([b]),) for b in p]
    return [b''.join(c) for c in itertools.product(*choices)]


def test_the_references_agree_where_their_meanings_coincide(judged):
    compared = 0
    for case, refs in judged:
        singles = case.ids + [p for p, _ in case.anchored] + case.anchored_word[0] + [segs[0] for segs, _, _ in case.glob]
        for s in singles:
            plain = refs.ids.search_ids(s)
            assert same(refs.glob.search_seq_ids([s], 0), plain), (case.seed, s)
            assert same(refs.terms.search_all_ids(([s], [])), plain), (case.seed, s)
            for anchors, word in ((START, 'start'), (END, 'end'), (START | END, 'entry')):
                assert same(refs.glob.search_seq_ids([s], anchors), refs.anchored.search_ids(s, word)), (case.seed, s, word)
            compared += 1
        for p in case.icase + case.ids:
            folded = refs.icase.search_icase_ids(p)
            letters = sum(F.is_letter(b) for b in p)
            if letters == 0:
                assert same(folded, refs.ids.search_ids(p)), (case.seed, p)
            if letters <= 6:
                union = sorted(set().union(*[refs.ids.search_ids(v).tolist() for v in all_spellings(p)]))
                assert same(folded, union), (case.seed, p)
                compared += 1
        for segs, _, _ in case.glob:
            if len(segs) >= 2:
                a, b = segs[0], segs[1]
                assert set(refs.glob.search_seq_ids([a, b], 0).tolist()) <= set(refs.terms.search_all_ids(([a, b], [])).tolist()), (case.seed, a, b)
                compared += 1
    assert compared > 3000
