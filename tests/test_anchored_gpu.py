"""Anchored search (Reader.search_anchored_batch_packed / search_anchored_ids_batch / count_anchored_bytes and the str
conveniences) against the brute-force reference of tests/anchored_ref.py.  Every query of every case is compared:
  * per query, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result (offsets and data), and every entry's
    text is the reference's for its id;
  * the batch took the general pipeline with the ANCHORED bit and none of MID, SMALL_*, RESIDENT, SA_ORDER.
The cases: the two ends of a chunk (first entry of the first and of later chunks, one-entry chunks, text without a
closing newline, the whole chunk as the pattern, a pattern longer than the chunk), matches that are not anchored, the
empty pattern and patterns with a newline, pattern lengths around the 8-byte key sample, more kept hits than one scan
workgroup and than the mid pipeline hold, work that follows the answer (last_stats()['hits']), batch shapes and the three
interval routes, placement (two parts on one device, a shard, a suffix array on the host tier, order='sa', no line table
before the id variant runs), errors, and the conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests import search_harness as H
from tests.anchored_ref import AnchoredRef
from tests.search_harness import FILLER, R, device_reader, filler, make_index, per_row as per_query

pytestmark = pytest.mark.gpu

KINDS = ('start', 'end', 'entry')


def all_kinds(patterns):
    """Every pattern under every anchor, as one mixed batch."""
    pats = [p for p in patterns for _ in KINDS]
    return pats, [k for _ in patterns for k in KINDS]


def check(r, ref, patterns, anchors, **kw):
    """patterns under anchors (one word, or one per pattern) on reader r against ref (the chunks r holds).  The batches
    compared here are the only ones that show PSS_ROUTE_ANCHORED to the route record of tests/search_harness.py."""
    return H.check(H.ANCHORED, r, ref, (list(patterns), anchors), **kw)


# ---- chunk edges -------------------------------------------------------------------------------------------------

def test_first_entry_of_every_chunk(tmp_path):
    """The entry at offset 0 of a chunk has no newline before it: chunk 0 and every later chunk."""
    rng = np.random.default_rng(41)
    lines = [b'HEAD%03d=' % i + filler(rng, int(rng.integers(0, 30))) for i in range(400)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'heads', data, 1500)
    ref = AnchoredRef.from_index(p)
    assert len(ref.chunks) >= 4 and sum(len(ch.text) for ch in ref.chunks) == len(data)
    firsts = [ch.entry(0) for ch in ref.chunks]
    lasts = [ch.entry(ch.num_entries - 1) for ch in ref.chunks]
    r = pysubstringsearch.Reader(p)
    try:
        pats, kinds = all_kinds(firsts + [f[:7] for f in firsts] + lasts + [x[-5:] for x in lasts] + [b'HEAD', b'HEAD0', b'EAD', b''])
        res = per_query(check(r, ref, pats, kinds))
        for c, ch in enumerate(ref.chunks):
            first = np.uint64(ch.index << 32)
            assert first in res[3 * c] and first in res[3 * c + 2]                              # whole entry: start, entry
            assert first in res[3 * (len(firsts) + c)] and first not in res[3 * (len(firsts) + c) + 2]      # 'HEADnnn': a prefix only
    finally:
        r.close()


def test_chunks_handed_over_on_the_device():
    """One-entry chunks, text without a closing newline (the tail under 'end' and 'entry'), the whole chunk as the pattern
    (n == m) and patterns longer than the chunk."""
    texts = [b'ONLYONE\n', b'first\nmid\nmid\nNOEND', b'NOEND', b'\n', b'x', b'ab\n\nab', b'mid\nmid', b'\n\nq']
    ref = AnchoredRef(texts)
    assert ref.chunks[1].num_entries == 4 and ref.chunks[2].num_entries == 1 and ref.chunks[7].num_entries == 3
    r = device_reader(texts)
    try:
        pats, kinds = all_kinds([b'ONLYONE', b'ONLY', b'ONE', b'ONLYONE\n', b'ONLYONEX', b'NOEND', b'NOEN', b'OEND', b'END', b'D', b'N',
                                 b'XNOEND', b'NOENDX', b'first', b'mid', b'mi', b'id', b'd', b'x', b'xx', b'ab', b'a', b'b', b'q', b'',
                                 b'first\nmid\nmid\nNOEND', b'first\nmid\nmid\nNOENDlonger than any chunk'])
        res = per_query(check(r, ref, pats, kinds))
        at = {p: 3 * i for i, p in enumerate(pats[::3])}
        # the tail of chunk 1 (line 3) and the whole of chunk 2, under 'end' and 'entry'
        for k in (1, 2):
            assert sorted(res[at[b'NOEND'] + k].tolist()) == [(1 << 32) | 3, 2 << 32]
        assert sorted(res[at[b'OEND'] + 1].tolist()) == [(1 << 32) | 3, 2 << 32] and res[at[b'OEND'] + 2].size == 0
        assert all(res[at[b'NOENDX'] + k].size == 0 and res[at[b'XNOEND'] + k].size == 0 for k in range(3))
        # the engine's entry rule: an unterminated last entry is handed out without its last byte; the id names the whole
        assert r.entries_by_id([(1 << 32) | 3, 2 << 32, (6 << 32) | 1]) == [b'NOEN', b'NOEN', b'mi']
        assert sorted(res[at[b'mid'] + 2].tolist()) == [(1 << 32) | 1, (1 << 32) | 2, 6 << 32, (6 << 32) | 1]
    finally:
        r.close()


# ---- not anchored means not returned -------------------------------------------------------------------------------

def test_unanchored_occurrences_are_not_returned(tmp_path):
    rng = np.random.default_rng(42)
    lines = [b'ab', b'abab', b'xab', b'abx', b'in the MIDDLE of it', b'TWICE and again TWICE', b'TWICETWICE', b'x TWICE',
             b'LEFT only', b'only RIGHT']
    lines += [filler(rng, int(rng.integers(0, 20))) for _ in range(200)]
    lines += [b'same entry'] * 500
    order = rng.permutation(len(lines))
    lines = [lines[int(i)] for i in order]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'unanch', data)
    ref = AnchoredRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        pats, kinds = all_kinds([b'ab', b'MIDDLE', b'TWICE', b'LEFT', b'RIGHT', b'same entry', b'same', b'entry', b'a', b'b', b'x'])
        res = per_query(check(r, ref, pats, kinds))
        at = {p: 3 * i for i, p in enumerate(pats[::3])}

        def texts(ids):
            return sorted(r.entries_by_id(ids))

        assert set(texts(res[at[b'ab'] + 2])) == {b'ab'}
        assert set(texts(res[at[b'ab']])) >= {b'ab', b'abab', b'abx'} and b'xab' not in texts(res[at[b'ab']])
        assert set(texts(res[at[b'ab'] + 1])) >= {b'ab', b'abab', b'xab'} and b'abx' not in texts(res[at[b'ab'] + 1])
        assert all(res[at[b'MIDDLE'] + k].size == 0 for k in range(3))                     # mid-entry only
        assert texts(res[at[b'TWICE']]) == [b'TWICE and again TWICE', b'TWICETWICE']       # at the start and again later: once
        assert texts(res[at[b'TWICE'] + 1]) == [b'TWICE and again TWICE', b'TWICETWICE', b'x TWICE']
        assert res[at[b'same entry'] + 2].size == 500 and np.unique(res[at[b'same entry'] + 2]).size == 500
        assert r.count(b'TWICE'.decode()) == 3
    finally:
        r.close()


# ---- empty and degenerate patterns ----------------------------------------------------------------------------------

@pytest.mark.parametrize('close', [True, False])
def test_empty_pattern_and_patterns_with_a_newline(tmp_path, close):
    """Runs of empty entries, an empty first entry (text[0] == '\\n') and an empty last entry; with a closing newline
    through the Writer, without one through the device hand-over (the last entry is then 'z')."""
    rng = np.random.default_rng(43)
    parts = [b'', b'', b'after two empties']
    for _ in range(30):
        parts += [filler(rng, int(rng.integers(1, 12)))] + [b''] * int(rng.integers(0, 4))
    parts += [b''] * 300 + [b'before the end', b'', b'']
    data = b'\n'.join(parts) + b'\n'
    assert data[0] == 0x0A and data.endswith(b'\n\n\n')
    if close:
        p = make_index(tmp_path, 'empties', data)
        ref = AnchoredRef.from_index(p)
        assert [ch.text for ch in ref.chunks] == [data]
        r = pysubstringsearch.Reader(p)
    else:
        data += b'z'
        ref = AnchoredRef([data])
        r = device_reader([data])
    try:
        nl_pats = [b'\n', b'\nafter', b'after\ntwo', b'end\n', b'\n\n', b'a\nb', b'\nz', b'z\n']
        pats, kinds = all_kinds([b''] + nl_pats + [b'after two empties', b'before the end', b'z'])
        res = per_query(check(r, ref, pats, kinds))
        total = ref.num_entries()
        assert total == len(parts) + (0 if close else 1)
        assert res[0].size == res[1].size == total                                          # b'' under start and end: every entry
        assert res[2].size == sum(1 for x in parts if not x)                                # ... under entry: the empty ones
        assert set(r.entries_by_id(res[2])) == {b''}
        for i in range(len(nl_pats)):
            assert all(res[3 * (1 + i) + k].size == 0 for k in range(3)), nl_pats[i]
    finally:
        r.close()


# ---- pattern lengths around the 8-byte key sample -------------------------------------------------------------------

def test_pattern_lengths_around_the_key_sample(tmp_path, search_env):
    """Patterns of 0, 1, 6, 7, 8, 9 and 300 bytes, present and absent: the rewritten queries are 1 .. 2 bytes longer, on
    both sides of the 8 bytes a key sample holds.  A dense sample table (one per 4 suffixes) puts several samples inside
    every interval."""
    search_env(PSS_SAMPLE_SHIFT=2)
    rng = np.random.default_rng(44)
    lens = (0, 1, 6, 7, 8, 9, 300)
    lines = []
    for _ in range(40):
        for m in lens:
            lines.append(filler(rng, m))
            lines.append(filler(rng, m) + filler(rng, int(rng.integers(1, 12))))
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'lens', data, 20000)
    ref = AnchoredRef.from_index(p)
    assert len(ref.chunks) >= 2
    present = []
    for m in lens:
        own = [x for x in lines if len(x) == m][:3]
        longer = [x for x in lines if len(x) > m][:3]
        present += own + [x[:m] for x in longer] + [x[len(x) - m:] for x in longer]
    absent = [x[:-1] + b'Z' for x in present if x] + [b'Z' + x[1:] for x in present if x]
    r = pysubstringsearch.Reader(p)
    try:
        pats, kinds = all_kinds(present + absent)
        res = per_query(check(r, ref, pats, kinds))
        assert r.last_stats()['route'] & R['KEY_SAMPLES']
        assert all(res[3 * i].size or res[3 * i + 1].size for i in range(len(present)))
        assert all(x.size == 0 for x in res[3 * len(present):])
    finally:
        r.close()


# ---- more kept hits than one scan workgroup and than the mid pipeline's 65 536 ---------------------------------------

def test_more_entries_than_the_mid_pipeline_holds(tmp_path):
    rng = np.random.default_rng(45)
    k = 70000
    raw = np.full((k, 3), 0x0A, dtype=np.uint8)
    raw[:, :2] = np.frombuffer(FILLER, np.uint8)[rng.integers(0, 4, (k, 2))]
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = AnchoredRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        res = per_query(check(r, ref, [b'', b'a', b'b', b'ab', b'q'], 'start', texts=False))
        assert res[0].size == k > 65536 and np.array_equal(np.sort(res[0]), np.arange(k, dtype=np.uint64))
        assert res[1].size > k // 5 and res[4].size == 0
        res = per_query(check(r, ref, [b'', b'a', b'ab'], ['end', 'end', 'entry'], texts=False))
        assert res[0].size == k
    finally:
        r.close()


# ---- work follows the answer ----------------------------------------------------------------------------------------

def test_hits_follow_the_answer_not_the_occurrences(tmp_path):
    """'a' occurs about 50 times in every entry and starts few of them: the anchored batch looks at one hit per
    matching entry, the unanchored count at every occurrence.  Both figures come from the text."""
    rng = np.random.default_rng(46)
    lines = []
    for i in range(300):
        body = np.frombuffer(b'ab', np.uint8)[rng.integers(0, 2, 100)].tobytes()
        lines.append((b'a' if i % 25 == 0 else b'b') + body)
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'work', data)
    ref = AnchoredRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    matching = int(ref.search_ids(b'a', 'start').size)
    occurrences = data.count(b'a')
    assert matching == 12 and occurrences >= 20 * matching
    r = pysubstringsearch.Reader(p)
    try:
        check(r, ref, [b'a'], 'start')
        assert r.count_anchored_bytes([b'a'], 'start') == [matching]
        assert r.last_stats()['hits'] == matching
        assert len(r.search_anchored_batch_packed([b'a'], 'start').counts) == 1 and r.last_stats()['hits'] == matching
        assert r.count_multiple_bytes([b'a']) == [len(lines)]
        assert r.last_stats()['hits'] == occurrences >= 20 * matching
    finally:
        r.close()


# ---- batch shape ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(47)
    lines = [filler(rng, int(rng.integers(0, 10))) for _ in range(600)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = AnchoredRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, lines


def test_batch_shapes(shape_index):
    p, ref, lines = shape_index
    rng = np.random.default_rng(48)
    r = pysubstringsearch.Reader(p)
    try:
        for k in KINDS:
            res = check(r, ref, [], k)
            assert res.ids.size == 0 and res.counts.size == 0
            res = check(r, ref, [b'MISS', b'\x01', b'zzzz', b'Z' * 40], k)
            assert res.ids.size == 0 and res.counts.tolist() == [0, 0, 0, 0]
        # one batch mixing the three anchors over the same patterns == three separate batches
        base = [b'', b'a', b'ab', b'abc', b'p'] + [lines[int(i)] for i in rng.integers(0, len(lines), 40)] + [filler(rng, 2) for _ in range(40)]
        pats, kinds = all_kinds(base)
        mixed = per_query(check(r, ref, pats, kinds, interval=R['INTERVAL_WAVE']))
        for j, k in enumerate(KINDS):
            alone = per_query(check(r, ref, base, k, interval=R['INTERVAL_WAVE']))
            assert all(np.array_equal(a, b) for a, b in zip(alone, mixed[j::3])), k
    finally:
        r.close()


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """3 000 queries on one chunk take the 16-lane interval search; the switches force the other two."""
    p, ref, lines = shape_index
    search_env(**env)
    rng = np.random.default_rng(49)
    base = [lines[int(i)][:int(rng.integers(0, 6))] for i in rng.integers(0, len(lines), 500)]
    base += [lines[int(i)][-int(rng.integers(1, 6)):] for i in rng.integers(0, len(lines), 400)] + [filler(rng, 3) for _ in range(100)]
    pats, kinds = all_kinds(base)
    assert len(pats) == 3000
    r = pysubstringsearch.Reader(p)
    try:
        check(r, ref, pats, kinds, interval=R[route])
    finally:
        r.close()


# ---- placement ------------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(50)
    lines = [b'HEAD%03d' % i if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = AnchoredRef.from_index(p)
    assert len(ref.chunks) >= 5
    base_pats = [b'', b'a', b'ab', b'HEAD', b'p'] + [ch.entry(0) for ch in ref.chunks] + [lines[int(i)] for i in rng.integers(0, len(lines), 30)]
    H.placement(H.ANCHORED, p, all_kinds(base_pats), search_env, ref=ref)


# ---- errors ---------------------------------------------------------------------------------------------------------

def test_bad_anchors(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        for bad in (0, 4, [0], [4], ['start', 4]):
            for call in (r.search_anchored_batch_packed, r.search_anchored_ids_batch, r.count_anchored_bytes):
                with pytest.raises(ValueError, match='anchor'):
                    call([b'a', b'b'][:len(bad) if isinstance(bad, list) else 2], bad)
        # through the C ABI: PSS_EINVAL with a message, *out untouched
        offs = (ctypes.c_uint64 * 3)(0, 1, 2)
        counts = (ctypes.c_uint64 * 2)(7, 7)
        for bad in (0, 4, 255):
            anc = (ctypes.c_uint8 * 2)(1, bad)
            for fn in (_ffi.lib.pss_reader_search_anchored_batch, _ffi.lib.pss_reader_search_anchored_ids_batch):
                out = ctypes.c_void_p()
                assert fn(r._handle(), b'ab', offs, 2, anc, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value
                assert f'anchors[1] = {bad}' in _ffi.last_error()
            assert _ffi.lib.pss_reader_count_anchored_batch(r._handle(), b'ab', offs, 2, anc, counts) == _ffi.PSS_EINVAL
            assert list(counts) == [7, 7] and f'anchors[1] = {bad}' in _ffi.last_error()
        anc = (ctypes.c_uint8 * 2)(1, 2)
        assert _ffi.lib.pss_reader_search_anchored_batch(r._handle(), b'ab', offs, 2, anc, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_anchored_batch(r._handle(), b'ab', offs, 2, None, ctypes.byref(ctypes.c_void_p())) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_count_anchored_batch(r._handle(), b'ab', offs, 2, anc, None) == _ffi.PSS_EINVAL
        check(r, ref, [b'a', b'b'], ['start', 'end'])           # the reader still answers
    finally:
        r.close()


# ---- the conveniences -----------------------------------------------------------------------------------------------

def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    w.add_entry('some short string')
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert r.search('short') == ['some short string']
        assert r.search_prefix('some') == ['some short string'] and r.search_prefix('short') == []
        assert r.search_suffix('string') == ['some short string'] and r.search_suffix('short') == []
        assert r.search_exact('some short string') == ['some short string'] and r.search_exact('some short strin') == []
        assert r.search_prefix('') == r.search_suffix('') == ['some short string'] and r.search_exact('') == []
        assert r.has_entries(['some short string', 'short', '', 'some short string\n']) == [True, False, False, False]
        assert r.has_entries([]) == []
        with pytest.raises(TypeError):
            r.search_prefix(b'some')
    finally:
        r.close()
