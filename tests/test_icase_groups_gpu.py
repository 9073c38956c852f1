"""Case-insensitive all-terms and wildcard search (the ``icase=True`` form of Reader.search_all_* / search_glob_* and the
six pss_reader_*_icase_* calls under them) against the brute-force reference of tests/icase_groups_ref.py.  Every group
or pattern of every batch goes through one check() per kind:
  * per group, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk the suffix-array order of the driver term's seed
    occurrence inside each entry's leftmost folded match of the driver term (the reference picks the driver by seed
    occurrences and sorts the suffixes themselves);
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result, and every entry's text is the
    reference's for its id;
  * on all three call forms the batch took the general pipeline -- GENERAL | interval bits (| COUNTS) and nothing else --
    and `hits` is the reference's sum of the drivers' seed occurrences, `entries` what came back, `queries` the groups.
The cases: meaning; the three-level indexing (group -> terms -> spellings) over several chunks; the driver by seed hits;
the verify step under fold at every position and length; what does not fold; exclusions; the dedupe; the glob's anchors,
order and overlap; equivalences with the exact-byte and the plain case-insensitive calls; more candidates than the mid
pipeline holds; the interval routes; placement; errors."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, glob_escape, glob_parse, icase_variants
from tests import search_harness as H
from tests.icase_groups_ref import IcaseGroupsRef
from tests.icase_ref import folded_occurrences
from tests.icase_texts import PAIRS_0X20, mangle, mixed_case_lines
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_group

pytestmark = pytest.mark.gpu


def check(kind, r, ref, batch, **kw):
    """batch (groups for kind 'all', glob patterns for kind 'glob') on reader r against ref (the chunks r holds)."""
    return H.check(H.ICASE_ALL if kind == 'all' else H.ICASE_GLOB, r, ref, list(batch), **kw)


def chunks_of(lines_per_chunk, closed=True):
    """(reader, reference) of chunks handed over on the device; closed = False leaves the LAST chunk without its newline."""
    texts = [b'\n'.join(lines) + b'\n' for lines in lines_per_chunk]
    if not closed:
        texts[-1] = texts[-1][:-1]
    assert all(len(t) < 1_000_000 for t in texts)
    return device_reader(texts), IcaseGroupsRef(texts)


def shuffled(rng, lines):
    return [lines[int(i)] for i in rng.permutation(len(lines))]


# ---- 1. meaning ---------------------------------------------------------------------------------------------------------

def test_meaning_all_terms():
    rng = np.random.default_rng(301)
    err, tmo, rty = (b'Error', b'ERROR', b'error', b'eRrOr'), (b'timeout', b'TIMEOUT', b'TimeOut'), (b'retry', b'RETRY', b'reTRy')
    lines = []
    for e in err:
        for t in tmo:
            lines += [e + b': ' + t, t + b' after ' + e, e + b' ' + t + b' ' + rty[len(lines) % 3], rty[len(lines) % 3] + b' ' + t + b' ' + e]
        lines += [e, e + b' only, RETRY', e + b' time out']
    lines += [b'timeout', b'retry', b'TIMEOUT RETRY', b'terror timeouts', b'ERR0R TIMEOUT']
    lines += [filler(rng, int(rng.integers(0, 30))) for _ in range(200)]
    r, ref = chunks_of([shuffled(rng, lines)])
    try:
        groups = [([b'Error', b'TIMEOUT'], [b'retry']), ([b'error', b'timeout'], []), [b'TIMEOUT', b'ERROR'], ([b'eRROR'], [b'Timeout']),
                  ([b'error'], [b'retry']), ([b'error'], [b'RETRY']), ([b'retry', b'error'], [b'timeout']), [b'error', b'nope'],
                  ([b'timeout'], [b'error', b'retry'])]
        res = per_group(check('all', r, ref, groups))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        assert len(res[0]) == 2 * len(err) * len(tmo) + 1 and b'terror timeouts' in texts(res[0])
        assert all(b'retry' not in t.lower() and b'error' in t.lower() and b'timeout' in t.lower() for t in texts(res[0]))
        assert texts(res[1]) == texts(res[2]) and len(res[1]) == 4 * len(err) * len(tmo) + 1
        # an exclude term present only in the other case still excludes
        assert texts(res[4]) == texts(res[5]) and not any(b'RETRY' in t.upper() for t in texts(res[4])) and len(res[4]) > 10
        assert texts(res[6]) == sorted(e + b' only, RETRY' for e in err) and res[7].size == 0
        assert texts(res[8]) == [b'ERR0R TIMEOUT', b'timeout']
    finally:
        r.close()


def test_meaning_glob_on_the_readme_example():
    rng = np.random.default_rng(302)
    yes = [b'GET /x/admin/y 500', b'get /Admin 500', b'Get /a/b/ADMIN 500', b'GET /admin/ 500 500', b'geT  /aDmIn 500']
    no = [b'GET /admin 5000', b'POST /admin 500', b'FORGET /admin 500', b'GET /admi 500', b'GET/admin 500', b'GET /admin 50', b'GET /admin500',
          b'/admin GET 500', b'GET 500 /admin']
    lines = yes + no + [filler(rng, int(rng.integers(0, 30))) for _ in range(200)]
    r, ref = chunks_of([shuffled(rng, lines)])
    try:
        res = per_group(check('glob', r, ref, [b'get */ADMIN* 500', b'GET */admin* 500', b'*get */admin* 500*', b'get *500', b'a*A', b'ab*BA']))
        assert sorted(r.entries_by_id(res[0])) == sorted(yes) == sorted(r.entries_by_id(res[1]))
        assert len(res[2]) == len(yes) + 2
        assert r.search_glob('get */ADMIN* 500', icase=True) == [e.decode() for e in r.entries_by_id(res[0])] != r.search_glob('get */ADMIN* 500')
        assert r.count_glob('get */ADMIN* 500', icase=True) == len(yes) and r.count_glob('get */ADMIN* 500') == 0
        assert r.count_all(['GET', '/ADMIN'], ['post'], icase=True) == len(yes) + len(no) - 2 and r.count_all(['GET', '/ADMIN'], ['post']) == 0
        assert sorted(r.search_all(['forget'], icase=True)) == ['FORGET /admin 500']
    finally:
        r.close()


def test_glob_contract_examples():
    r, ref = chunks_of([[b'a', b'A', b'aa', b'aA', b'aBa', b'abBA', b'ABba', b'abxba', b'aba', b'ab', b'ba']])
    try:
        res = per_group(check('glob', r, ref, [b'a*A', b'ab*BA', b'A', b'*AB*BA*', b'aB']))
        assert sorted(r.entries_by_id(res[0])) == [b'ABba', b'aA', b'aBa', b'aa', b'abBA', b'aba', b'abxba']   # not `a`, not `A`
        assert sorted(r.entries_by_id(res[1])) == [b'ABba', b'abBA', b'abxba']                            # not `aBa`
        assert sorted(r.entries_by_id(res[2])) == [b'A', b'a'] and sorted(r.entries_by_id(res[4])) == [b'ab']
        assert sorted(r.entries_by_id(res[3])) == [b'ABba', b'abBA', b'abxba']                            # overlapping placement: no match
    finally:
        r.close()


# ---- 2. three levels: group -> terms -> spellings, over several chunks ----------------------------------------------------

def test_three_level_indexing(tmp_path, search_env):
    """Terms of 1, 2, 32 and 64 spellings in one batch over >= 3 chunks; the driver as first, middle and last term of its
    group; a driver that changes from chunk to chunk; no driver's term index equals its group's index."""
    search_env(PSS_ICASE_SEED_LETTERS=6)
    rng = np.random.default_rng(303)
    common = [b'12', b'a1', b'abcde', b'abcdef', b'mnop', b'34 56']
    n = 700
    lines = []
    for i in range(n):
        words = [common[int(k)] for k in rng.integers(0, len(common), int(rng.integers(1, 5)))]
        if i % 23 == 0:
            words.insert(int(rng.integers(0, len(words) + 1)), b'rare9z')
        # `early` is frequent in the first half and seldom in the second, `late` the other way round
        if rng.random() < (0.5 if i < n // 2 else 0.03):
            words.append(b'early')
        if rng.random() < (0.03 if i < n // 2 else 0.5):
            words.append(b'late')
        lines.append(mangle(rng, b' '.join(words), 0.4))
    p = make_index(tmp_path, 'levels', b'\n'.join(lines) + b'\n', 3000)
    ref = IcaseGroupsRef.from_index(p)
    assert len(ref.chunks) >= 3
    assert [len(icase_variants(t)[1]) for t in (b'12', b'a1', b'abcde', b'abcdef')] == [1, 2, 32, 64]
    groups = [[b'abcdef', b'A1', b'RARE9Z'], [b'12', b'rare9z', b'abcde'], [b'Rare9Z', b'abcdef', b'mnop'], [b'EARLY', b'LATE'],
              ([b'12', b'34 56'], [b'a1']), ([b'abcdef', b'a1'], [b'MNOP', b'12']), [b'34 56'], [b'abcdef', b'12', b'mnop', b'a1', b'abcde'],
              ([b'abcde'], [b'abcdef', b'rare9z'])]
    r = pysubstringsearch.Reader(p)
    try:
        res = check('all', r, ref, groups)
        assert res.ids.size > 200 and all(c > 0 for c in res.counts.tolist()[:8])
        drivers = [ref.drivers('all', g) for g in groups]
        assert set(drivers[0]) == {2} and set(drivers[1]) == {1} and set(drivers[2]) == {0}
        assert len(set(drivers[3]) - {None}) == 2                              # the driver differs between chunks of one group
        first_term = np.cumsum([0] + [len(g[0]) + len(g[1]) if isinstance(g, tuple) else len(g) for g in groups])
        for g, ds in enumerate(drivers):
            assert all(d is None or first_term[g] + d != g for d in ds), g
        chunk_of = (res.ids >> np.uint64(32)).astype(np.int64)
        group_of = np.repeat(np.arange(len(groups)), res.counts.astype(np.int64))
        assert (np.diff(chunk_of)[np.diff(group_of) == 0] >= 0).all() and np.unique(chunk_of).size >= 3       # chunk-major inside a group
        globs = [b'*abcdef*A1*', b'*12*rare9z*', b'Rare9Z*', b'*EARLY*LATE', b'*34 56', b'abcdef*12*mnop*', b'*a1*abcde*abcdef*12*', b'12']
        res = check('glob', r, ref, globs)
        assert res.ids.size > 50 and sum(c > 0 for c in res.counts.tolist()) >= 6
    finally:
        r.close()


# ---- 3. the driver: by seed hits ------------------------------------------------------------------------------------------

def test_the_driver_is_chosen_by_seed_hits():
    """`abcdezz` is the rarer TERM, but its seed `abcde` is commoner than `mnop`: `mnop` drives.  The second chunk lacks
    `mnop` altogether: its pairs contribute no hit, though `abcdezz` is there."""
    rng = np.random.default_rng(304)
    one = [mangle(rng, b'abcdexx ' + filler(rng, 5)) for _ in range(60)] + [mangle(rng, b'x mnop ' + filler(rng, 4)) for _ in range(20)]
    one += [b'ABCDEzz and MNop', b'mnop abcdeZZ', b'abcdezz alone', b'mnOP abcdez']
    two = [mangle(rng, b'abcdexx') for _ in range(10)] + [b'abcdezz mno p', b'ABCDEZZ']
    r, ref = chunks_of([shuffled(rng, one), shuffled(rng, two)])
    try:
        assert icase_variants(b'abcdezz')[0] == 0 and icase_variants(b'abcdezz')[1][0] == b'ABCDE'
        text = ref.chunks[0].text
        assert folded_occurrences(text, b'abcdezz') == 3 < folded_occurrences(text, b'mnop') == 23 < folded_occurrences(text, b'abcde') == 64
        group, glob = [b'abcdezz', b'mnop'], b'*abcdezz*MNOP*'
        assert ref.drivers('all', group) == [1, None] and ref.drivers('glob', glob) == [1, None]
        assert ref.hits('all', [group]) == 23 and ref.hits('all', [[b'abcdezz']]) == 64 + 12
        res = per_group(check('all', r, ref, [group, [b'abcdezz'], [b'mnop', b'abcdezz']]))
        assert sorted(r.entries_by_id(res[0])) == [b'ABCDEzz and MNop', b'mnop abcdeZZ'] and len(res[1]) == 5
        res = per_group(check('glob', r, ref, [glob, b'*MNOP*abcdezz*']))
        assert r.entries_by_id(res[0]) == [b'ABCDEzz and MNop'] and r.entries_by_id(res[1]) == [b'mnop abcdeZZ']
    finally:
        r.close()


# ---- 4. the verify step under fold ------------------------------------------------------------------------------------------

KEY = b'~k~'
LONG = (b'qrstuvwxyz0123456789' * 7)[:137]
WORDS = [b'q', b'qrstuvw', b'qrstuvwx', b'qrstuvwxy', b'qrstuvwxyz012345', b'qrstuvwxyz0123456', LONG]


def test_a_non_driver_term_at_every_position():
    """Per word (1, 7, 8, 9, 16, 17 and 137 bytes): candidates of the driver `~k~` that hold the word at start position
    0 .. 65 in some spelling, and beside each a near miss with the word's last byte changed.  Lines of 0 .. 3 bytes in
    front shift the entries against the 8-byte grid.  Then the word ending exactly at the entry's end, at n of the
    unterminated last chunk, and a word longer than its entry.  70 entries per word hold it without the key, so the
    key is the driver."""
    rng = np.random.default_rng(305)
    chunks, expect = [], {}
    for w in WORDS:
        lines, good = [], 0
        miss = w[:-1] + b'#'
        for pos in range(66):
            for body, ok in ((mangle(rng, w), True), (mangle(rng, miss), False)):
                lines += [b'%' * ((pos + ok) % 4), filler(rng, pos) + body + filler(rng, int(rng.integers(0, 9))) + b' ' + KEY]
                good += ok
        lines += [KEY + b' ' + mangle(rng, w), KEY + filler(rng, 3) + mangle(rng, miss), KEY + b' ' + w[:-1], KEY, mangle(rng, w) + KEY]
        good += 2
        lines += [filler(rng, int(rng.integers(0, 40))) + mangle(rng, w) for _ in range(70)]
        lines.append(KEY + b' ' + w.upper())                               # the last entry: closed in every chunk but the last
        good += 1
        expect[w] = good
        chunks.append(lines)
    r, ref = chunks_of(chunks, closed=False)
    try:
        assert ref.chunks[-1].text.endswith(LONG.upper()) and len(LONG) > 128
        groups = [[w, KEY] for w in WORDS]
        for g in groups:
            assert all(d in (1, None) for d in ref.drivers('all', g)) and ref.drivers('all', g).count(1) >= 1
        res = per_group(check('all', r, ref, groups))
        for w, got in zip(WORDS, res):
            assert got.size >= expect[w], w
        assert res[-1].size == expect[LONG]                                     # nothing else holds the long word
        # the same candidates walked in order: the word in front of the key, and the key in front of a word at the end
        globs = [b'*' + w + b'*' + KEY for w in WORDS] + [KEY + b'*' + w for w in WORDS] + [b'*' + w + KEY + b'*' for w in WORDS]
        res = per_group(check('glob', r, ref, globs))
        assert res[len(WORDS) - 1].size == 66 + 1 and res[2 * len(WORDS) - 1].size == 2 and res[3 * len(WORDS) - 1].size == 1
    finally:
        r.close()


# ---- 5. what does not fold ----------------------------------------------------------------------------------------------------

def test_bytes_that_differ_by_0x20_and_are_no_letters():
    lines = []
    for lo, hi in PAIRS_0X20:
        lines += [b'key x' + lo + b'y', b'KEY X' + hi + b'Y', b'pad ' + lo + lo + hi + b' key', lo, hi, lo + lo, hi + hi, b'x' + lo, b'X' + hi]
    r, ref = chunks_of([lines])
    try:
        esc = glob_escape
        groups, globs = [], []
        for lo, hi in PAIRS_0X20:
            groups += [[b'key', b'X' + lo + b'Y'], [b'KEY', b'x' + hi + b'y'], [b'key', lo + lo + hi], [b'key', hi + hi + lo], ([b'kEy'], [b'x' + lo])]
            globs += [b'key*X' + esc(lo) + b'Y', b'KEY*x' + esc(hi) + b'y', b'*' + esc(lo + lo + hi) + b'*key', b'*' + esc(hi + hi + lo) + b'*key',
                      b'key x' + esc(lo) + b'Y']
        res = per_group(check('all', r, ref, groups))
        for k, (lo, hi) in enumerate(PAIRS_0X20):
            a, b, aab, bba, ex = res[5 * k:5 * k + 5]
            assert r.entries_by_id(a) == [b'key x' + lo + b'y'] and r.entries_by_id(b) == [b'KEY X' + hi + b'Y'], (lo, hi)
            assert r.entries_by_id(aab) == [b'pad ' + lo + lo + hi + b' key'] and bba.size == 0, (lo, hi)
            assert b'key x' + lo + b'y' not in r.entries_by_id(ex) and b'KEY X' + hi + b'Y' in r.entries_by_id(ex), (lo, hi)
        res = per_group(check('glob', r, ref, globs))
        for k, (lo, hi) in enumerate(PAIRS_0X20):
            a, b, aab, bba, eq = res[5 * k:5 * k + 5]
            assert r.entries_by_id(a) == [b'key x' + lo + b'y'] == r.entries_by_id(eq) and r.entries_by_id(b) == [b'KEY X' + hi + b'Y'], (lo, hi)
            assert r.entries_by_id(aab) == [b'pad ' + lo + lo + hi + b' key'] and bba.size == 0, (lo, hi)
    finally:
        r.close()


def test_zero_in_a_term_does_not_match_the_padding():
    texts = [b'ka\x00y\nbkA', b'kA', b'ka\x00', b'\x00ak\nkA\x00\n\x00']
    r, ref = device_reader(texts), IcaseGroupsRef(texts)
    try:
        res = per_group(check('all', r, ref, [[b'K', b'a\x00'], [b'k', b'A\x00\x00'], [b'k', b'A\x00\x00\x00\x00\x00\x00\x00\x00'], [b'\x00', b'K'],
                                              ([b'k'], [b'a\x00'])]))
        assert res[0].tolist() == [0, 2 << 32, (3 << 32) | 1] and res[1].size == 0 and res[2].size == 0
        assert sorted(res[4].tolist()) == [1, 1 << 32, 3 << 32]
        res = per_group(check('glob', r, ref, [b'*k*A\x00', b'*ka\x00*', b'ka\x00\x00', b'*A\x00\x00', b'k*\x00']))
        assert res[0].tolist() == [2 << 32, (3 << 32) | 1] and res[2].size == 0 and res[3].size == 0
    finally:
        r.close()


# ---- 6. exclusions ------------------------------------------------------------------------------------------------------------

def test_exclusions():
    rng = np.random.default_rng(306)
    one = [b'alpha beta', b'ALPHA Beta GAMMA', b'Alpha', b'alpha gammas', b'beta gamma', b'aLPHa gamm a']
    one += [filler(rng, int(rng.integers(0, 20))) for _ in range(50)]
    two = [b'ALPHA', b'alpha BETA', b'beta'] + [filler(rng, int(rng.integers(0, 20))) for _ in range(50)]      # no `gamma` here
    r, ref = chunks_of([shuffled(rng, one), shuffled(rng, two)])
    try:
        assert ref.seed_hits(1, b'gamma') == 0 and ref.seed_hits(0, b'gammaray') == 3          # the seed of `gammaray` is `gamma`
        groups = [([b'alpha'], [b'GAMMA']), ([b'alpha'], [b'gammaray']), ([b'ALPHA'], [b'x\ny']), [b'alpha'], ([b'alpha'], [b'beta', b'Gamma']),
                  ([b'alpha'], [b'alpha']), ([b'alpha', b'BETA'], [b'gamma'])]
        res = per_group(check('all', r, ref, groups))
        assert len(res[0]) == 3 + 2 and len(res[1]) == 5 + 2                 # seed present, term absent: nothing excluded
        assert res[2].tolist() == res[3].tolist() and len(res[3]) == 7      # a void exclude term is ignored
        assert sorted(r.entries_by_id(res[4])) == [b'ALPHA', b'Alpha', b'aLPHa gamm a'] and res[5].size == 0
        assert sorted(r.entries_by_id(res[6])) == [b'alpha BETA', b'alpha beta']
        # a void include term: a count of 0 and not one hit looked at
        for batch in ([[b'alpha', b'a\nb']], [[b'a\nb', b'alpha']], [([b'\n'], [b'alpha'])]):
            assert check('all', r, ref, batch).ids.size == 0
            assert r.last_stats()['hits'] == 0
        assert check('glob', r, ref, [b'alpha*\n*', b'*a\nb']).ids.size == 0 and r.last_stats()['hits'] == 0
    finally:
        r.close()


# ---- 7. the dedupe ------------------------------------------------------------------------------------------------------------

def test_the_driver_twice_in_one_entry_in_two_spellings():
    rng = np.random.default_rng(307)
    lines = [b'error .. ERROR timeout', b'ERROR .. error TIMEOUT', b'Error error ERROR eRROR timeout', b'x ERROR y Error z', b'timeout ERROR error']
    lines += [mangle(rng, b'timeout ' + filler(rng, 6)) for _ in range(30)] + [filler(rng, int(rng.integers(0, 20))) for _ in range(50)]
    r, ref = chunks_of([shuffled(rng, lines)])
    try:
        assert ref.drivers('all', [b'timeout', b'error']) == [1]
        res = per_group(check('all', r, ref, [[b'timeout', b'error'], [b'error']]))
        assert len(res[0]) == 4 and len(res[1]) == 5
        st = r.last_stats()
        assert st['hits'] == 12 + 12 and st['entries'] == 9
        res = per_group(check('glob', r, ref, [b'*error*timeout', b'*timeout*ERROR*', b'*error*error*']))
        assert len(res[0]) == 3 and r.entries_by_id(res[1]) == [b'timeout ERROR error'] and len(res[2]) == 5
    finally:
        r.close()


# ---- 8. the glob: anchors, the driver's place, overlap, leftmost-greedy ---------------------------------------------------------

SEGS = [b'ab', b'cd9', b'ef', b'gh7']


def test_glob_anchors_and_segment_counts():
    rng = np.random.default_rng(308)
    lines = []
    for _ in range(400):
        parts = []
        for s in SEGS:
            if rng.random() < 0.25:
                parts.append(filler(rng, int(rng.integers(1, 4))).replace(b'a', b'm').replace(b'c', b'm').replace(b'e', b'm').replace(b'g', b'm'))
            if rng.random() < 0.8:
                parts.append(mangle(rng, s))
        lines.append(b''.join(parts))
    lines += [b'ab', b'AB', b'abCD9', b'ABcd9EFgh7', b'abab', b'cd9ab', b'xAB CD9 ab', b'AB ab', b'aba', b'a b']
    closed = shuffled(rng, lines)
    r, ref = chunks_of([closed, [b'xx ab CD9', b'Ab', b'zz AB cd9 ef GH7']], closed=False)
    try:
        globs = []
        for k in (1, 2, 4):
            body = b'*'.join(SEGS[:k])
            globs += [body, b'*' + body, body + b'*', b'*' + body + b'*']
        res = per_group(check('glob', r, ref, globs))
        assert all(len(x) > 0 for x in res)
        for k in range(3):
            both, end, start, none = (set(x.tolist()) for x in res[4 * k:4 * k + 4])
            assert both <= end <= none and both <= start <= none and both < none and (k == 2 or end != start)
        last = (1 << 32) | 2                                                    # the unterminated last entry: its last byte takes part
        assert last in res[9].tolist() and last not in res[10].tolist() and (1 << 32) in res[5].tolist()
        # leftmost-greedy under fold: the first segment's leftmost occurrence is `AB`, not the pattern's `ab`
        res = per_group(check('glob', r, ref, [b'*ab*cd9*', b'*ab*ab*', b'*AB*BA*', b'*ab*cd9']))
        assert b'xAB CD9 ab' in r.entries_by_id(res[0]) and b'AB ab' in r.entries_by_id(res[1]) and b'aba' not in r.entries_by_id(res[2])
        assert (1 << 32) in res[3].tolist()
    finally:
        r.close()


def test_glob_driver_first_middle_last():
    rng = np.random.default_rng(309)
    lines = []
    for i in range(300):
        words = [mangle(rng, w) for w in (b'ab', b'cd9') if rng.random() < 0.7]
        if i % 10 == 0:
            words.insert(int(rng.integers(0, len(words) + 1)), mangle(rng, b'rare9z'))
        lines.append(b' '.join(words))
    r, ref = chunks_of([lines[:150], lines[150:]])
    try:
        globs = [b'*RARE9Z*ab*cd9*', b'*ab*Rare9z*cd9*', b'*ab*cd9*rare9Z*', b'rare9z*', b'*rare9z', b'*ab*cd9*']
        assert [set(ref.drivers('glob', g)) for g in globs[:3]] == [{0}, {1}, {2}]
        res = per_group(check('glob', r, ref, globs))
        assert all(len(x) > 0 for x in res)
    finally:
        r.close()


def test_one_segment_with_both_anchors_is_search_exact_under_fold():
    rng = np.random.default_rng(310)
    lines = [b'Hello', b'HELLO', b'hello', b'hELLo', b'hello!', b' hello', b'hell', b'hello hello', b'HELLO', b'h*llo', b'H*LLO']
    lines += [mangle(rng, filler(rng, 5)) for _ in range(100)]
    r, ref = chunks_of([shuffled(rng, lines), [b'HellO', b'x']], closed=False)
    try:
        for word in (b'hello', b'h*llo'):
            got = check('glob', r, ref, [glob_escape(word)])
            exact = r.search_anchored_ids_batch(icase_variants(word, 6)[1], 'entry')
            assert np.array_equal(np.sort(got.ids), np.sort(exact.ids)) and got.ids.size == (6 if word == b'hello' else 2)
        # prefix and suffix under fold, spelled with glob_escape
        res = per_group(check('glob', r, ref, [glob_escape(b'hello') + b'*', b'*' + glob_escape(b'HELLO')]))
        assert len(res[0]) == 6 + 2 and len(res[1]) == 6 + 2
    finally:
        r.close()


# ---- 9. equivalences ----------------------------------------------------------------------------------------------------------

def test_letterless_groups_are_the_exact_byte_search():
    rng = np.random.default_rng(311)
    abc = np.frombuffer(b'0123 _-=a', np.uint8)
    lines = [bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 20)))]) for _ in range(500)]
    r, ref = chunks_of([lines[:250], lines[250:]])
    try:
        groups = [[b'1', b'2'], ([b'12'], [b'0 ']), [b'_-', b'=', b'3'], ([b' '], [b'99', b'1']), [b'0123'], [b'3', b'2', b'1', b'0']]
        got, exact = check('all', r, ref, groups), r.search_all_ids_batch(groups)
        assert np.array_equal(got.ids, exact.ids) and np.array_equal(got.counts, exact.counts) and got.ids.size > 200
        globs = [b'*1*2*', b'12*', b'*_-*=*3', b'*0 *', b'0123*_', b'*3*2*1*0*']
        got, exact = check('glob', r, ref, globs), r.search_glob_ids_batch(globs)
        assert np.array_equal(got.ids, exact.ids) and np.array_equal(got.counts, exact.counts) and got.ids.size > 100
    finally:
        r.close()


def test_one_term_is_the_plain_case_insensitive_search(search_env):
    rng = np.random.default_rng(312)
    lines = mixed_case_lines(rng, 500, 0, 30) + [b'USER_ID=12345678', b'x ABCDEFGH', b'abcdefgh here']
    r, ref = chunks_of([lines[:250], lines[250:]])
    try:
        words = [b'ab', b'ABC', b'p', b'mnop', b'NOPE', b'abcdefgh', b'user_id=12345678', b'h HERE', b'12', b' ']
        plain = r.search_icase_ids_batch(words)
        got = check('all', r, ref, [[w] for w in words])
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts) and got.ids.size > 200
        got = check('glob', r, ref, [b'*' + glob_escape(w) + b'*' for w in words])
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts)
        # every seed length gives the same id sets
        groups = [[b'abcdefgh', b'here'], ([b'a', b'B'], [b'p']), [b'user_id', b'12345678'], ([b'abc'], [b'mn']), [b'AB', b'c']]
        globs = [b'*abcdefgh*HERE', b'x*abcdefgh', b'*a*B*c*', b'user_id=*', b'*ab*C*']
        base = None
        for F in (5, 1, 2, 3, 4, 6):
            search_env(PSS_ICASE_SEED_LETTERS=F)
            sets = [np.sort(x).tolist() for x in per_group(check('all', r, ref, groups)) + per_group(check('glob', r, ref, globs))]
            base = sets if base is None else base
            assert sets == base, F
        assert sum(len(x) for x in base) > 20
    finally:
        r.close()


def test_a_batch_of_one_segment_globs_keeps_its_anchors():
    """Every pattern has one segment, so the batch has as many terms as groups -- the shape of a plain case-insensitive
    batch, which skips the all-terms verify.  A sequence batch never may: its anchors are checked there."""
    rng = np.random.default_rng(315)
    lines = mixed_case_lines(rng, 400, 0, 30) + [b'ab xYz7 cd', b'q XYZ7 r', b'mn xyz7xyz7 op', b'Ab', b'aB at the start', b'at the end AB']
    lines = shuffled(rng, lines)
    r, ref = chunks_of([lines[:200], lines[200:]])
    try:
        words = [b'xyz7', b'AB', b'p', b'mno', b'Nope', b'a*b']
        batch = [pre + glob_escape(w) + post for w in words for pre, post in ((b'', b''), (b'', b'*'), (b'*', b''), (b'*', b'*'))]
        assert all(len(glob_parse(p)[0]) == 1 for p in batch) and {glob_parse(p)[1] for p in batch} == {0, 1, 2, 3}
        counts = check('glob', r, ref, batch).counts.tolist()
        by_word = dict(zip(words, zip(*[iter(counts)] * 4)))            # (p, p*, *p, *p*) per word
        assert by_word[b'xyz7'] == (0, 0, 0, 3)                         # (only in the middle of its entries)
        assert by_word[b'AB'][0] >= 1 and by_word[b'AB'][0] < by_word[b'AB'][1] < by_word[b'AB'][3] > by_word[b'AB'][2]
        assert any(c[1] != c[3] for c in by_word.values())
    finally:
        r.close()


def test_one_term_groups_alone_and_beside_a_two_term_group():
    """A batch of one-term groups skips the all-terms verify, the same groups beside a two-term group run it: the same ids
    in the same order either way, and those of the plain case-insensitive call."""
    rng = np.random.default_rng(316)
    lines = mixed_case_lines(rng, 400, 0, 30) + [b'x ABCDEFGH', b'abcdefgh here', b'ABCDE only', b'xx abcdeg', b'aBcDe']
    lines = shuffled(rng, lines)
    r, ref = chunks_of([lines[:200], lines[200:]])
    try:
        words = [b'ab', b'ABC', b'p', b'abcdefgh', b'ab\ncd', b'NOPE', b'h HERE', b' ']
        singles = [[w] for w in words]
        plain = r.search_icase_ids_batch(words)
        alone = r.search_all_ids_batch(singles, icase=True)
        st = r.last_stats()
        assert st['hits'] > st['entries'] > 100                         # (the seed `abcde` occurs where `abcdefgh` does not)
        assert alone.counts.tolist() == r.count_all_bytes(singles, icase=True) == r.count_icase_bytes(words)
        alone = check('all', r, ref, singles)
        beside = check('all', r, ref, singles + [[b'ab', b'C']])
        assert beside.counts.tolist()[:len(words)] == alone.counts.tolist() == plain.counts.tolist()
        assert np.array_equal(beside.ids[:alone.ids.size], alone.ids) and np.array_equal(alone.ids, plain.ids)
        assert alone.counts[words.index(b'ab\ncd')] == 0 and alone.counts[words.index(b'abcdefgh')] == 2
        assert beside.counts[-1] > 0
    finally:
        r.close()


# ---- 10. more candidates than the mid pipeline's 65 536 -------------------------------------------------------------------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    """100 000 entries of ten bytes, each with `qrstu` in some spelling -- the driver, 100 000 seed hits -- and a tail of
    `vvvv` in some spelling (three overlapping occurrences of `vv`: the commoner seed) or `wxyz`."""
    rng = np.random.default_rng(313)
    k = 100_000
    raw = np.empty((k, 10), dtype=np.uint8)
    raw[:, 9] = 0x0A
    raw[:, 0:5] = np.frombuffer(b'qrstu', np.uint8) ^ (rng.integers(0, 2, (k, 5)).astype(np.uint8) << 5)
    which = rng.integers(0, 3, k)
    raw[:, 5:9] = np.frombuffer(b'wxyz', np.uint8)
    vv = np.frombuffer(b'vvvv', np.uint8) ^ (rng.integers(0, 2, (k, 4)).astype(np.uint8) << 5)
    raw[which < 2, 5:9] = vv[which < 2]
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = IcaseGroupsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        assert ref.drivers('all', [b'VV', b'qrstu']) == [1]
        res = check('all', r, ref, [[b'VV', b'qrstu']], texts=False, order=False)
        assert r.last_stats()['hits'] == k > 65536                     # every entry is a candidate
        assert np.array_equal(np.sort(res.ids), np.flatnonzero(which < 2).astype(np.uint64)) and res.ids.size > k // 2
        res = check('glob', r, ref, [b'QRSTU*vv'], texts=False, order=False)
        assert r.last_stats()['hits'] == k and res.ids.size == int((which < 2).sum())
    finally:
        r.close()


# ---- 11. the interval routes ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(314)
    lines = mixed_case_lines(rng, 600, 0, 16)
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('gshape'), 'gshape', data)
    ref = IcaseGroupsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, lines


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """75 groups of two terms of three to seven letters on one chunk expand to 2 048 .. 8 191 spellings and take the
    16-lane interval search; the switches force the other two."""
    p, ref, lines = shape_index
    search_env(PSS_ICASE_SEED_LETTERS=None, **env)
    rng = np.random.default_rng(315)
    groups, globs = [], []
    while len(groups) < 75:
        ln = lines[int(rng.integers(0, len(lines)))]
        n, m = int(rng.integers(3, 8)), int(rng.integers(3, 8))
        if len(ln) >= n + m:
            at = int(rng.integers(0, len(ln) - n - m + 1))
            a, b = mangle(rng, ln[at:at + n]), mangle(rng, ln[at + n:at + n + m])
            groups.append([b, a])
            globs.append(b'*' + glob_escape(a) + b'*' + glob_escape(b) + b'*')
    nvar = sum(len(icase_variants(t)[1]) for g in groups for t in g)
    assert 2048 <= nvar < 8192
    r = pysubstringsearch.Reader(p)
    try:
        res = check('all', r, ref, groups, interval=R[route])
        assert res.ids.size >= 75 and (res.counts > 0).all()
        res = check('glob', r, ref, globs, interval=R[route])
        assert res.ids.size >= 75 and (res.counts > 0).all()
    finally:
        r.close()


# ---- 12. placement ------------------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(316)
    lines = [mangle(rng, b'HEAD%03d ' % i + filler(rng, 6)) if i % 40 == 0 else mangle(rng, filler(rng, int(rng.integers(0, 24))), 0.3)
             for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'gplace', data, 4000)
    ref = IcaseGroupsRef.from_index(p)
    assert len(ref.chunks) >= 5
    groups = [[b'ab', b'CD'], ([b'head'], [b'1']), [b'HEAD0', b'a'], ([b'p', b'O'], [b'ab', b'cd']), [b'MISSING', b'a'], [b'12', b'ead'],
              ([b'abc'], [b'head', b'p'])]
    globs = [b'head*', b'*HEAD0*a*', b'*ab*cd*', b'*p', b'a*B*c*', b'*missing*', b'*d1*']
    globs += [glob_escape(ch.entry(0).swapcase()) for ch in ref.chunks if ch.entry(0)]              # the entry at offset 0 of every chunk
    for i in rng.integers(0, len(lines), 20):
        ln = lines[int(i)]
        if len(ln) >= 8:
            groups.append([ln[1:4].swapcase(), ln[4:8].swapcase()])
            globs.append(b'*' + ln[1:4].swapcase() + b'*' + ln[5:8].swapcase() + b'*')

    # devices=[0, 0]: the merge is part-major inside a group, so the stated order is not compared there
    assert H.placement(H.ICASE_ALL, p, groups, search_env, order_multi=False, ref=ref).ids.size > 50
    assert H.placement(H.ICASE_GLOB, p, globs, search_env, order_multi=False, ref=ref).ids.size > 50


# ---- 13. errors -----------------------------------------------------------------------------------------------------------------

def test_errors(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        before = check('all', r, ref, [[b'ab', b'C']])
        for call in (r.search_all_ids_batch, r.search_all_batch_packed, r.count_all_bytes):
            for bad in ([[b'']], [[b'ab', b'']], [([b'a'], [b''])], [[]], [([], [b'a'])]):
                with pytest.raises(ValueError):
                    call(bad, icase=True)
            for bad in ([b'ab'], ['ab'], [['ab']], [[None]], b'ab'):
                with pytest.raises(TypeError):
                    call(bad, icase=True)
            with pytest.raises(TypeError):
                call([[b'ab']], icase=1)
        for call in (r.search_glob_ids_batch, r.search_glob_batch_packed, r.count_glob_bytes):
            for bad in ([b''], [b'*'], [b'ab', b'**']):
                with pytest.raises(ValueError):
                    call(bad, icase=True)
            for bad in (b'ab', 'ab', ['ab'], [None]):
                with pytest.raises(TypeError):
                    call(bad, icase=True)
            with pytest.raises(TypeError):
                call([b'ab'], icase='yes')
        # through the C ABI with a reader: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        blob, offs = b'abc', np.array([0, 2, 2, 3], dtype=np.uint64)
        goff, flags = np.array([0, 1, 3], dtype=np.uint64), np.zeros(3, dtype=np.uint8)
        empty_group = np.array([0, 3, 3], dtype=np.uint64)
        good = np.array([0, 1, 2, 3], dtype=np.uint64)
        lib = _ffi.lib
        for fn, noun in ((lib.pss_reader_search_terms_icase_batch, 'term'), (lib.pss_reader_search_terms_icase_ids_batch, 'term'),
                         (lib.pss_reader_search_seq_icase_batch, 'segment'), (lib.pss_reader_search_seq_icase_ids_batch, 'segment')):
            out = ctypes.c_void_p()
            assert fn(h, blob, offs.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
            assert not out.value and f'{noun} 1 is empty' in _ffi.last_error()
            assert fn(h, blob, good.ctypes.data, 3, empty_group.ctypes.data, 2, flags.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
            assert not out.value and 'group 1 has no' in _ffi.last_error()
            assert fn(h, blob, good.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, None) == _ffi.PSS_EINVAL
        for fn, noun in ((lib.pss_reader_count_terms_icase_batch, 'term'), (lib.pss_reader_count_seq_icase_batch, 'segment')):
            counts = np.full(4, 7, dtype=np.uint64)
            assert fn(h, blob, offs.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and f'{noun} 1 is empty' in _ffi.last_error()
        # ... and a good batch goes through the same calls; the reader still answers, and its statistics are the good batch's
        out = ctypes.c_void_p()
        assert lib.pss_reader_search_terms_icase_batch(h, blob, good.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data,
                                                       ctypes.byref(out)) == _ffi.PSS_OK and out.value
        want = ref.search_all_ids([b'A']).size + ref.search_all_ids([b'B', b'C']).size
        assert lib.pss_result_num_entries(out) == want > 0 and r.last_stats()['entries'] == want and r.last_stats()['queries'] == 2
        lib.pss_result_free(out)
        out = ctypes.c_void_p()
        anch = np.array([0, 1], dtype=np.uint8)
        assert lib.pss_reader_search_seq_icase_ids_batch(h, blob, good.ctypes.data, 3, goff.ctypes.data, 2, anch.ctypes.data,
                                                         ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert lib.pss_result_num_entries(out) == ref.search_glob_ids(b'*A*').size + ref.search_glob_ids(b'B*C*').size
        lib.pss_result_free(out)
        again = check('all', r, ref, [[b'ab', b'C']])
        assert np.array_equal(again.ids, before.ids)
        # the exact-byte calls and the plain case-insensitive call answer as before
        assert r.count_all_bytes([[b'ab', b'C']]) == [sum(1 for ln in lines if b'ab' in ln and b'C' in ln)]
        assert r.count_icase_bytes([b'ab']) == [sum(1 for ln in lines if b'ab' in ln.lower())]
    finally:
        r.close()


@pytest.mark.parametrize('kind', [H.ICASE_ALL, H.ICASE_GLOB], ids=lambda kind: kind.name)
def test_rows_and_term_bytes_around_a_multiple_of_64(kind):
    """63, 64 and 65 groups whose term bytes add up to 31, 32 and 33 modulo 64, in the other case, on one chunk and on three
    (search_harness.layout_edges)."""
    swapped = lambda groups: [(a.swapcase(), b.swapcase(), ab) for a, b, ab in groups]
    if kind is H.ICASE_ALL:
        H.layout_edges(kind, lambda groups: [[a, b] for a, b, _ in swapped(groups)], min_ids=63)
    else:
        H.layout_edges(kind, lambda groups: H.edge_globs(swapped(groups)), min_ids=63)
