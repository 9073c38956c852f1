"""All-terms search (Reader.search_all_ids_batch / search_all_batch_packed / count_all_bytes and the str conveniences)
against the brute-force reference of tests/all_terms_ref.py.  Every group of every batch goes through one check():
  * per group, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result (offsets and data), and every entry's
    text is the reference's for its id;
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), none of ANCHORED, MID, SMALL_*, RESIDENT,
    SA_ORDER.
The cases: what "all and none" means (order inside the entry, overlapping and repeated terms, include == exclude, groups of
1 to 8 terms in one batch), chunk edges (device hand-over: offset 0, one-entry chunks, no closing newline, 0x00 against
the padding, 0x0A terms, terms in different chunks), work that follows the rarest term (last_stats()['hits']) and the
tie rule, entry and term lengths around the 8- and 64-byte load widths with near misses, more candidates than the mid
pipeline and one scan workgroup hold, batch shapes and the three interval routes, placement (two parts on one device, a
shard, a suffix array on the host tier, order='sa', no line table before the id variant runs), errors, conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests import search_harness as H
from tests.all_terms_ref import AllTermsRef, split_group
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_group

pytestmark = pytest.mark.gpu


def check(r, ref, groups, **kw):
    """groups on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.ALL_TERMS, r, ref, list(groups), **kw)


# ---- 1. meaning ---------------------------------------------------------------------------------------------------

def test_meaning(tmp_path):
    rng = np.random.default_rng(61)
    lines = [b'ERROR then TIMEOUT', b'TIMEOUT then ERROR', b'ERROR alone', b'TIMEOUT alone', b'ERROR ERROR twice', b'ERROR TIMEOUT RETRY',
             b'RETRY ERROR', b'ABAB', b'ABA', b'BAB', b'xABAB', b'WHOLE ENTRY', b'WHOLE ENTRY and more', b'T1 T2 T3 T4 T5 T6 T7 T8',
             b'T1 T2 T3 T4 T5 T6 T7', b'T8 T7 T6 T5 T4 T3 T2 T1 RETRY', b'T1', b'']
    lines += [filler(rng, int(rng.integers(0, 30))) for _ in range(300)]
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'meaning', data)
    ref = AllTermsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    ts = [b'T%d' % i for i in range(1, 9)]
    groups = [
        [b'ERROR', b'TIMEOUT'], [b'TIMEOUT', b'ERROR'], [b'ERROR'], [b'TIMEOUT'], [b'ERROR ERROR'], [b'ERROR', b'ERROR ERROR'],
        [b'ABA', b'BAB'], [b'BAB', b'ABA'], ([b'ABA'], [b'BAB']), ([b'BAB'], [b'ABA']), [b'AB', b'BA', b'ABAB'],
        [b'WHOLE ENTRY', b'WHOLE'], [b'WHOLE', b'WHOLE ENTRY'], ([b'WHOLE ENTRY'], [b'more']), [b'ERROR', b'ERROR'], [b'ERROR'] * 5,
        ([b'ERROR'], [b'ERROR']), ([b'ERROR', b'TIMEOUT'], [b'TIMEOUT']), ([b'ERROR'], [b'RETRY']), ([b'ERROR'], [b'R']),
        ([b'ERROR'], [b'never there']), ([b'ERROR', b'TIMEOUT'], [b'RETRY']), ([b'ERROR'], [b'RETRY', b'TIMEOUT', b'twice', b'alone']),
        ([b'a'], [b'b']), ([b'a', b'b'], [b'c', b'd']), [b'a', b'b', b'c'], [b'never there'], [b'ERROR', b'never there'],
    ] + [ts[:k] for k in range(1, 9)] + [(ts[:k], [b'RETRY']) for k in range(1, 9)] + [ts[::-1]]
    assert sorted({len(split_group(g)[0]) + len(split_group(g)[1]) for g in groups})[:8] == list(range(1, 9))
    r = pysubstringsearch.Reader(p)
    try:
        res = per_group(check(r, ref, groups))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        assert texts(res[0]) == texts(res[1]) == [b'ERROR TIMEOUT RETRY', b'ERROR then TIMEOUT', b'TIMEOUT then ERROR']
        assert texts(res[4]) == texts(res[5]) == [b'ERROR ERROR twice']
        assert texts(res[6]) == texts(res[7]) == texts(res[10]) == [b'ABAB', b'xABAB'] and texts(res[8]) == [b'ABA'] and texts(res[9]) == [b'BAB']
        assert texts(res[13]) == [b'WHOLE ENTRY'] and np.array_equal(res[14], res[2]) and np.array_equal(res[15], res[2])
        assert res[16].size == res[17].size == res[19].size == 0 and np.array_equal(res[20], res[2]) and 0 < res[18].size < res[2].size
        assert texts(res[28 + 7]) == [b'T1 T2 T3 T4 T5 T6 T7 T8', b'T8 T7 T6 T5 T4 T3 T2 T1 RETRY'] and texts(res[36 + 7]) == [b'T1 T2 T3 T4 T5 T6 T7 T8']
        # a group of one include term is the plain id search, array for array
        singles = [b'ERROR', b'a', b'ab', b'T1', b'never there', b'WHOLE ENTRY', b'p']
        got, plain = check(r, ref, [[t] for t in singles]), r.search_ids_batch(singles)
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts)
    finally:
        r.close()


# ---- 2. chunk edges -------------------------------------------------------------------------------------------------

def test_chunk_edges_handed_over_on_the_device():
    texts = [b'ONLYONE x\n',                         # 0: a one-entry chunk
             b'first x\n\n\nab\nmid x\nx NOEND',      # 1: the entry at offset 0, empty entries, a short entry, no closing newline
             b'NOEND',                               # 2: the whole chunk is one unterminated entry
             b'\n', b'x',                            # 3, 4
             b'xb\x00y\nab',                         # 5: a real 0x00, and 'b' as the very last byte before the padding
             b'b',                                   # 6
             b'ONLYA here\nx\n', b'ONLYB here\nx\n',  # 7, 8: two terms that never share a chunk
             b'HEL\nLO x\nHELLO']                    # 9
    ref = AllTermsRef(texts)
    r = device_reader(texts)
    try:
        groups = [
            [b'first', b'x'], [b'x', b'first'], [b'ONLYONE', b'x'], [b'ONLYONE x', b'ONLYONE'], ([b'x'], [b'ONLYONE']),
            [b'mid', b'mid x'], [b'ab', b'mid'], [b'ab', b'abc'], [b'ab', b'a', b'b'],
            # the unterminated last entry: a term that ends at the very last byte, as include and as exclude, driving and verified
            [b'x', b'NOEND'], [b'NOEND', b'x'], [b'x', b'D'], ([b'x'], [b'NOEND']), ([b'x'], [b'D']), ([b'x'], [b'END']), [b'NOEND', b'NOEND'],
            ([b'NOEND'], [b'NOEND']), [b'NOEN', b'NOEND'], [b'N', b'OEND'], ([b'NOE'], [b'x']), [b'x', b'NOENDx'], [b'NOEND', b'NOEND\x00'],
            # 0x00: in the text it matches, against the zero padding behind the chunk it does not
            [b'b', b'b\x00'], [b'b\x00', b'b'], ([b'b'], [b'b\x00']), [b'a', b'b\x00'], [b'b', b'\x00'], ([b'b'], [b'\x00']), [b'b\x00\x00'],
            [b'x', b'x\x00'], ([b'x'], [b'x\x00']), [b'D', b'D\x00\x00\x00\x00\x00\x00\x00\x00\x00'],
            # 0x0A: an include term with one empties the group, an exclude term with one excludes nothing
            [b'x', b'\n'], [b'\n', b'x'], ([b'x'], [b'\n']), [b'HEL', b'HEL\nLO'], ([b'HEL'], [b'HEL\nLO']), [b'HEL\nLO'], ([b'LO'], [b'L\nL', b'\n\n']),
            [b'HEL', b'LO'], [b'HELLO', b'LO'], [b'x', b'x\n'], ([b'x'], [b'x\n']), [b'first x\n', b'first'],
            [b'ONLYA', b'here'], [b'ONLYB', b'here'], [b'here', b'x'],
        ]
        res = per_group(check(r, ref, groups))
        at = {repr(g): i for i, g in enumerate(groups)}
        noend = [(1 << 32) | 5, 2 << 32]
        assert res[at[repr([b'x', b'NOEND'])]].tolist() == [noend[0]] and sorted(res[at[repr([b'NOEND', b'NOEND'])]].tolist()) == noend
        assert sorted(res[at[repr([b'N', b'OEND'])]].tolist()) == noend and res[at[repr(([b'NOE'], [b'x']))]].tolist() == [2 << 32]
        assert (1 << 32) | 5 not in res[at[repr(([b'x'], [b'D']))]].tolist() and res[at[repr(([b'x'], [b'D']))]].size
        assert r.entries_by_id(noend) == [b'x NOEN', b'NOEN']          # handed out without the last byte, matched with it
        assert res[at[repr([b'b', b'b\x00'])]].tolist() == [5 << 32] and res[at[repr([b'b\x00\x00'])]].size == 0
        assert sorted(res[at[repr(([b'b'], [b'b\x00']))]].tolist()) == [(1 << 32) | 3, (5 << 32) | 1, 6 << 32]
        assert res[at[repr([b'x', b'\n'])]].size == res[at[repr([b'HEL\nLO'])]].size == 0
        assert np.array_equal(res[at[repr(([b'x'], [b'\n']))]], r.search_ids_batch([b'x']).ids)
        assert res[at[repr([b'HEL', b'LO'])]].tolist() == [(9 << 32) | 2]
        # two terms that occur only in different chunks: no hit is looked at
        got = check(r, ref, [[b'ONLYA', b'ONLYB'], [b'ONLYB here', b'ONLYA'], ([b'ONLYA', b'ONLYB'], [b'x'])])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
        assert r.count_all_bytes([[b'ONLYA', b'ONLYB']]) == [0] and r.last_stats()['hits'] == 0
    finally:
        r.close()


# ---- 3. the work follows the rarest term ----------------------------------------------------------------------------

def test_hits_follow_the_rarest_term(tmp_path):
    """'a' occurs about 50 times in each of 300 entries, 'RARE' once in 12 of them: whichever comes first in the group,
    the batch looks at the hits of RARE alone.  Both figures come from the text."""
    rng = np.random.default_rng(62)
    lines = []
    for i in range(300):
        body = np.frombuffer(b'ab', np.uint8)[rng.integers(0, 2, 100)].tobytes()
        lines.append(body[:40] + b'RARE' + body[40:] if i % 25 == 0 else body)
    # a tie: TIEX and TIEY occur twice each, in the same two entries, in opposite suffix order
    lines += [b'TIEX1 TIEY2', b'TIEX2 TIEY1']
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'work', data)
    ref = AllTermsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    rare = data.count(b'RARE')
    assert rare == 12 and data.count(b'TIEX') == data.count(b'TIEY') == 2
    r = pysubstringsearch.Reader(p)
    try:
        for group in ([b'a', b'RARE'], [b'RARE', b'a'], ([b'RARE', b'a'], [b'never there']), [b'a', b'b', b'RARE', b'ab']):
            got = check(r, ref, [group])
            assert got.ids.size == rare and r.last_stats()['hits'] == rare
            assert r.count_all_bytes([group]) == [rare] and r.last_stats()['hits'] == rare
            assert len(r.search_all_batch_packed([group]).counts) == 1 and r.last_stats()['hits'] == rare
        assert r.count_multiple_bytes([b'a']) == [300]
        assert r.last_stats()['hits'] == data.count(b'a') >= 20 * rare
        # equal counts: the include term with the lowest index drives, and its plain order is the group's
        x, y = r.search_ids_batch([b'TIEX']).ids, r.search_ids_batch([b'TIEY']).ids
        assert x.size == y.size == 2 and x.tolist() == y.tolist()[::-1]
        assert np.array_equal(check(r, ref, [[b'TIEX', b'TIEY']]).ids, x)
        assert np.array_equal(check(r, ref, [[b'TIEY', b'TIEX']]).ids, y)
        assert np.array_equal(check(r, ref, [([b'TIEY', b'TIEX', b'TIEY'], [b'RARE'])]).ids, y)
    finally:
        r.close()


# ---- 4. entry and term lengths around the load widths ----------------------------------------------------------------

ENTRY_LENS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 300, 5000)
TERM_LENS = (1, 7, 8, 9, 64, 300)


def test_entry_and_term_lengths_around_the_load_widths(tmp_path):
    """Every term T_m (a prefix of one 300-byte string over an alphabet the filler lacks, so T_7 is in T_8 is in T_9 ..)
    is planted in entries of every length that holds it: at the start, at the end, across an 8-byte and across a 64-byte
    position -- and so is its near miss, T_m with the last byte changed.  'Z' marks a third of those entries: as the only
    include term of ([Z], [T_m]) it drives and the verify step meets hits and near misses of every shape; '#' marks two
    entries in all (T_300 and its near miss at the end of 5000 bytes), fewer than any T_m has, so it also drives [#, T_m]; [T_m, T_m] makes the verify step find T_m in
    every entry the driver T_m found."""
    rng = np.random.default_rng(63)
    base = bytes(np.frombuffer(b'QRSTUVWXY', np.uint8)[rng.integers(0, 9, 300)])
    term = {m: base[:m] for m in TERM_LENS}
    miss = {m: base[:m - 1] + b'!' for m in TERM_LENS}
    lines = [filler(rng, n) for n in ENTRY_LENS for _ in range(2)]
    planted = 0
    for m in TERM_LENS:
        for n in ENTRY_LENS:
            if n < m:
                continue
            for at in sorted({0, n - m, max(0, min(n - m, 8 - m // 2 - 1)), max(0, min(n - m, 64 - m // 2 - 1))}):
                for t in (term[m], miss[m]):
                    e = bytearray(filler(rng, n))
                    e[at:at + m] = t
                    free = [i for i in range(n) if not at <= i < at + m]
                    if n == 5000 and m == 300 and at == n - m:
                        e[free[0]] = ord('#')
                    elif free and rng.integers(0, 3) == 0:
                        e[free[int(rng.integers(0, len(free)))]] = ord('Z')
                    lines.append(bytes(e))
                    planted += 1
    # a term present only across a newline, and self-overlapping prefixes
    lines += [b'abcHEL', b'LOdef', b'AAAAB', b'AAAA', b'B', b'AAAAAAAAAB', b'AAAAAAAA', b'AB', b'xAAABx Z', b'AAAAAAAAB Z', b'AAAAAAA!B Z']
    data = b'\n'.join(lines) + b'\n'
    assert planted > 300 and len(data) < 700_000
    p = make_index(tmp_path, 'widths', data)
    ref = AllTermsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    z = data.count(b'Z')
    assert z > 50 and data.count(b'#') == 2 < min(data.count(term[m]) for m in TERM_LENS)          # '#' drives every [#, T_m]
    groups = []
    for m in TERM_LENS:
        groups += [[term[m], term[m]], [b'Z', term[m]], ([b'Z'], [term[m]]), [b'Z', miss[m]], ([b'Z'], [miss[m]]), ([term[m]], [miss[m]]),
                   ([term[m]], [term[m]]), [miss[m], miss[m]], [b'#', term[m]], ([b'#'], [term[m]])]
    groups += [[term[a], term[b]] for a in TERM_LENS for b in TERM_LENS if a < b]
    groups += [[b'HEL', b'HELLO'], [b'LO', b'HELLO'], [b'abc', b'HEL', b'LO'], [b'A', b'AAAB'], [b'AAAB', b'AAAB'], [b'B', b'AAAAB'],
               [b'Z', b'AAAB'], [b'A', b'AAAAAAAAB'], [b'Z', b'AAAAAAAAB'], ([b'Z'], [b'AAAAAAAAB']), [b'AAAAAAAAB', b'AAAAAAAAAB']]
    r = pysubstringsearch.Reader(p)
    try:
        res = per_group(check(r, ref, groups))
        for k, m in enumerate(TERM_LENS):
            assert np.array_equal(np.sort(res[10 * k]), ref.search_ids(term[m])) and res[10 * k].size >= 3, m       # [T_m, T_m] loses nothing
            assert res[10 * k + 1].size + res[10 * k + 2].size == z and res[10 * k + 2].size and (res[10 * k + 1].size or m > 64), m
            assert res[10 * k + 6].size == 0 and res[10 * k + 8].size + res[10 * k + 9].size == 2
            assert res[10 * k + 8].size == (2 if m < 300 else 1), m             # the near miss of T_300 holds every shorter T_m
        at = len(groups) - 11
        assert res[at].size == res[at + 1].size == res[at + 2].size == 0                         # HELLO only across the newline
        assert sorted(r.entries_by_id(res[at + 3])) == [b'AAAAAAAAAB', b'AAAAAAAAB Z', b'AAAAB', b'xAAABx Z']
        assert sorted(r.entries_by_id(res[at + 6])) == [b'AAAAAAAAB Z', b'xAAABx Z']
        assert sorted(r.entries_by_id(res[at + 8])) == [b'AAAAAAAAB Z']
    finally:
        r.close()


# ---- 5. more candidates than the mid pipeline's 65 536 and than one scan workgroup -----------------------------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    rng = np.random.default_rng(64)
    k = 70000
    raw = np.full((k, 3), 0x0A, dtype=np.uint8)
    raw[:, 0] = ord('x')
    raw[:, 1] = np.frombuffer(b'ab', np.uint8)[rng.integers(0, 2, k)]
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = AllTermsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    half = data.count(b'a')
    assert k // 3 < half < 2 * k // 3
    r = pysubstringsearch.Reader(p)
    try:
        # 'x' drives all 70 000 entries where it is the only include term; 'a' is then verified in every one of them
        res = per_group(check(r, ref, [([b'x'], [b'a']), [b'x', b'x'], ([b'x'], [b'q'])], texts=False))
        assert r.last_stats()['hits'] == 3 * k
        assert res[0].size == k - half and res[1].size == res[2].size == k > 65536
        assert np.array_equal(np.sort(res[1]), np.arange(k, dtype=np.uint64))
        res = per_group(check(r, ref, [[b'x', b'a'], [b'xa', b'x'], ([b'x', b'a'], [b'xa']), [b'x', b'a', b'b']], texts=False))
        assert res[0].size == res[1].size == half and res[2].size == res[3].size == 0
        assert r.last_stats()['hits'] == 3 * half + min(half, k - half)
    finally:
        r.close()


# ---- 6. batch shapes and interval routes ------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(65)
    lines = [filler(rng, int(rng.integers(0, 10))) for _ in range(600)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = AllTermsRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, lines


def test_batch_shapes(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, [])
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_all_batch_packed([]).offsets.tolist() == [0] and r.count_all_bytes([]) == []
        res = check(r, ref, [[b'MISS'], [b'a', b'MISS'], [b'MISS', b'a'], ([b'\x01'], [b'a']), [b'Z' * 40, b'zz']])
        assert res.ids.size == 0 and res.counts.tolist() == [0] * 5 and r.last_stats()['hits'] == 0
        res = check(r, ref, [[b'a'], [b'MISS'], [b'a', b'b'], ([b'a'], [b'b'])], interval=R['INTERVAL_WAVE'])
        assert res.counts[0] == res.counts[2] + res.counts[3] > 0 and res.counts[1] == 0
    finally:
        r.close()


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """3 000 groups of one to three terms on one chunk (about 5 000 term pairs) take the 16-lane interval search; the
    switches force the other two."""
    p, ref, lines = shape_index
    search_env(**env)
    rng = np.random.default_rng(66)

    def piece():
        ln = lines[int(rng.integers(0, len(lines)))]
        if len(ln) < 2 or rng.integers(0, 8) == 0:
            return filler(rng, 2)
        a = int(rng.integers(0, len(ln) - 1))
        return ln[a:a + int(rng.integers(1, 4))]

    groups = []
    for i in range(3000):
        k = i % 3
        groups.append([piece()] if k == 0 else [piece(), piece()] if k == 1 else ([piece(), piece()], [piece()]))
    nterms = sum(len(split_group(g)[0]) + len(split_group(g)[1]) for g in groups)
    assert 2048 <= nterms < 8192
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, groups, interval=R[route])
        assert res.ids.size > 1000
    finally:
        r.close()


# ---- 7. placement -----------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(67)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = AllTermsRef.from_index(p)
    assert len(ref.chunks) >= 5
    groups = [[b'a', b'b'], [b'b', b'a'], ([b'a'], [b'b']), [b'HEAD', b'0'], ([b'HEAD'], [b'a', b'b']), [b'p'], [b'ab', b'cd'], [b'a', b'b', b'c', b'd'],
              [b'MISS', b'a'], ([b'e'], [b'f', b'g', b'h'])]
    groups += [[ch.entry(0), ch.entry(0)[:3] or b'a'] for ch in ref.chunks if ch.entry(0)]
    groups += [[lines[int(i)][:2], lines[int(i)][-2:]] for i in rng.integers(0, len(lines), 30) if len(lines[int(i)]) >= 2]
    assert H.placement(H.ALL_TERMS, p, groups, search_env, ref=ref).ids.size > 100


# ---- 8. errors --------------------------------------------------------------------------------------------------------

def c_batch(terms, goff, excl):
    blob = b''.join(terms)
    offs = np.cumsum([0] + [len(t) for t in terms]).astype(np.uint64)
    return blob, offs, np.array(goff, dtype=np.uint64), np.array(excl if excl else [0], dtype=np.uint8)


BAD_C_BATCHES = [
    ('no include term', [b'a', b'b'], [0, 1, 2], [0, 1]),
    ('no include term', [b'a'], [0, 0, 1], [0]),
    ('is empty', [b'a', b''], [0, 2], [0, 0]),
    ('exclude[1] = 2', [b'a', b'b'], [0, 2], [0, 2]),
    ('exclude[0] = 255', [b'a', b'b'], [0, 2], [255, 0]),
    ('group offsets', [b'a', b'b'], [1, 2], [0, 0]),
    ('group offsets', [b'a', b'b'], [0, 1], [0, 0]),
    ('group offsets', [b'a', b'b', b'c'], [0, 2, 1, 3], [0, 0, 0]),
    ('group offsets', [b'a', b'b'], [0, 3, 2], [0, 0]),
]


def test_errors(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        calls = (r.search_all_batch_packed, r.search_all_ids_batch, r.count_all_bytes)
        for bad, what in (([[]], 'no include term'), ([[b'a'], ([], [b'a'])], 'no include term'), ([[b'a', b'']], 'empty term'),
                          ([([b'a'], [b''])], 'empty term')):
            for call in calls:
                with pytest.raises(ValueError, match=what):
                    call(bad)
        with pytest.raises(ValueError, match='no include term'):
            r.search_all([], exclude=['a'])
        # through the C ABI: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        for what, terms, goff, excl in BAD_C_BATCHES:
            blob, offs, g, e = c_batch(terms, goff, excl)
            ng = len(goff) - 1
            for fn in (_ffi.lib.pss_reader_search_terms_batch, _ffi.lib.pss_reader_search_terms_ids_batch):
                out = ctypes.c_void_p()
                assert fn(h, blob, offs.ctypes.data, len(terms), g.ctypes.data, ng, e.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value and what in _ffi.last_error(), (what, _ffi.last_error())
            counts = np.full(4, 7, dtype=np.uint64)
            assert _ffi.lib.pss_reader_count_terms_batch(h, blob, offs.ctypes.data, len(terms), g.ctypes.data, ng, e.ctypes.data,
                                                         counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
        # a null out, null offsets, null flags
        blob, offs, g, e = c_batch([b'a', b'b'], [0, 2], [0, 1])
        args = (h, blob, offs.ctypes.data, 2, g.ctypes.data, 1, e.ctypes.data)
        assert _ffi.lib.pss_reader_search_terms_batch(*args, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_terms_ids_batch(*args, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_count_terms_batch(*args, None) == _ffi.PSS_EINVAL
        out = ctypes.c_void_p()
        assert _ffi.lib.pss_reader_search_terms_batch(h, blob, offs.ctypes.data, 2, None, 1, e.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_terms_batch(h, blob, offs.ctypes.data, 2, g.ctypes.data, 1, None, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_terms_batch(h, blob, None, 2, g.ctypes.data, 1, e.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert not out.value
        # ... and the good batch goes through the same call; the reader still answers
        assert _ffi.lib.pss_reader_search_terms_batch(*args, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == ref.search_all_ids(([b'a'], [b'b'])).size > 0
        _ffi.lib.pss_result_free(out)
        check(r, ref, [[b'a', b'b'], ([b'a'], [b'b'])])
    finally:
        r.close()


# ---- 9. the conveniences ----------------------------------------------------------------------------------------------

def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    w.add_entry('some short string')
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert r.search('short') == ['some short string']
        assert r.search_all(['short', 'some']) == r.search_all(['string']) == r.search_all(('some', 'some')) == ['some short string']
        assert r.search_all(['short', 'long']) == [] and r.search_all(['short'], exclude=['some']) == []
        assert r.search_all(['short'], exclude=['long']) == r.search_all(['short'], exclude=()) == ['some short string']
        assert r.count_all(['short', 'string']) == 1 and r.count_all(['short'], exclude=['string']) == 0 and r.count_all(['g', 'long']) == 0
        assert r.search_all(['some short string', 'g']) == ['some short string'] and r.search_all(['some short string\n']) == []
        for bad in (b'some', [b'some'], 'some'):
            with pytest.raises(TypeError):
                r.search_all(bad)
            with pytest.raises(TypeError):
                r.count_all(bad)
        with pytest.raises(TypeError):
            r.search_all(['some'], exclude=b'short')
        with pytest.raises(ValueError):
            r.search_all([])
        with pytest.raises(ValueError):
            r.search_all(['some', ''])
    finally:
        r.close()


def test_rows_and_term_bytes_around_a_multiple_of_64():
    """63, 64 and 65 groups whose term bytes add up to 31, 32 and 33 modulo 64, on one chunk and on three (search_harness.layout_edges)."""
    H.layout_edges(H.ALL_TERMS, lambda groups: [[a, b] for a, b, _ in groups], min_ids=63)
