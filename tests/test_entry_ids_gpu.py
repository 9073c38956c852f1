"""Entry ids (Reader.search_ids_batch / entries_by_id / entry_counts / entry_ordinals) against the brute-force reference of
tests/entry_id_ref.py.  Every query of every case is compared:
  * per query, the sorted ids equal the reference's, no id twice, counts equal count_multiple_bytes;
  * entry by entry, in order, entries_by_id_packed(search_ids_batch(qs).ids) is search_batch_packed(qs) -- for both result
    orders -- and every entry's text is the reference's for that id;
  * the batch took the general pipeline (last_stats()['route']) and reports entries / 8 bytes per entry.
The cases: the edges of rank / select (runs of empty entries, an entry over several blocks of the line table, entries
that start or end on a block edge, first / last entry, one-entry chunks, text without a closing newline, a replaced
chunk), line numbers of an indexed file, batch sizes (nothing, no hit, more kept hits than the mid pipeline holds),
placement (two parts on one device, a shard, a suffix array on the host tier), invalid ids, and laziness (a reader that
never asks for ids holds nothing for them)."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests import search_harness as H
from tests.entry_id_ref import IdRef
from tests.search_harness import FILLER, R, device_chunk, filler, make_index

pytestmark = pytest.mark.gpu

LINE_BLOCK = 256                # bytes of text per entry of the line table (search.h, kLineShift = 8)
EDGE = 1024                     # the largest block PSS_LINE_BLOCK_SHIFT allows: an edge of it is an edge of every size


def table_bytes(ref, block=LINE_BLOCK):
    """HBM the line tables of ref's chunks take ("Entry ids"): one u32 per block, the closing rank, the entry count."""
    return sum(((len(ch.text) + block - 1) // block + 2) * 4 for ch in ref.chunks if len(ch.text))


def check(r, ref, queries, **kw):
    """queries through search_ids_batch on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.PLAIN, r, ref, list(queries), **kw)


def edge_text(rng, close=True):
    """One chunk's worth of lines built around the edges of the line table."""
    parts = []

    def add(line):
        parts.append(line + b'\n')

    def size():
        return sum(map(len, parts))

    add(b'FIRSTENTRY ' + filler(rng, 5))                       # the first entry of the chunk
    for _ in range(40):
        add(filler(rng, int(rng.integers(0, 40))))
    add(b'BEFOREEMPTY')
    for _ in range(2500):                                      # a run of empty entries over more than two blocks of 1024
        add(b'')
    add(b'AFTEREMPTY')
    add(b'LONGHEAD' + filler(rng, 5000) + b'LONGTAIL')         # an entry over several blocks: blocks without a newline
    add(b'AFTERLONG')
    add(filler(rng, (-size() - 1) % EDGE))                     # its newline is the last byte of a block ...
    assert size() % EDGE == 0
    add(b'EDGESTART ' + filler(rng, 30))                       # ... so this entry starts on the block edge
    add(filler(rng, (-size()) % EDGE + EDGE - 7) + b'EDGEEND')  # this one ends with a block: its newline opens the next
    assert size() % EDGE == 1
    add(b'AFTEREDGE')
    add(b'TWICE ' + filler(rng, 9) + b' TWICE')                # holds the pattern twice (the result orders differ here)
    add(b'x TWICE')
    add(b'TWICETWICE')
    for _ in range(60):
        add(filler(rng, int(rng.integers(0, 300))))
    add(b'LASTENTRY')                                          # the last entry of the chunk
    data = b''.join(parts)
    return data if close else data[:-1]


EDGE_QUERIES = [b'', b'\n', b'\n\n', b'\n\n\n', b'FIRSTENTRY', b'FIRST', b'BEFOREEMPTY', b'BEFOREEMPTY\n\n', b'AFTEREMPTY',
                b'\nAFTEREMPTY', b'\n\nAFTEREMPTY\n', b'LONGHEAD', b'LONGTAIL', b'LONGTAIL\n', b'LONGTAIL\nAFTERLONG', b'AFTERLONG',
                b'EDGESTART', b'\nEDGESTART', b'EDGEEND', b'EDGEEND\n', b'EDGEEND\nAFTEREDGE', b'AFTEREDGE', b'TWICE', b'TWICET',
                b'E', b'LASTENTRY', b'LASTENTRY\n', b'LASTENTR', b'Y', b'a', b'ab', b'p\n', b'\na', b'abcdefgh', b'MISSING', b'\x00']


@pytest.mark.parametrize('order', ['text', 'sa'])
@pytest.mark.parametrize('shift', [None, 6, 10])
def test_rank_select_edges(tmp_path, search_env, order, shift):
    search_env(PSS_LINE_BLOCK_SHIFT=shift)
    rng = np.random.default_rng(11)
    data = edge_text(rng)
    p = make_index(tmp_path, 'edge', data)
    ref = IdRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p, order=order)
    try:
        res = check(r, ref, EDGE_QUERIES)
        every = res.ids[:res.counts[0]]                          # the empty query: every entry, once
        assert np.array_equal(np.sort(every), np.arange(data.count(b'\n'), dtype=np.uint64))
        assert r.entry_counts == {0: data.count(b'\n')}
        # single queries; a low-latency reader answers ids the ordinary way
        for low in (False, True):
            r.set_low_latency(low)
            for q in ('FIRSTENTRY', 'TWICE', 'LASTENTRY', '', 'EDGESTART', 'nothing here'):
                got = r.search_ids(q)
                assert np.array_equal(np.sort(got), ref.search_ids(q.encode())), q
                assert r.last_stats()['route'] & R['GENERAL']
                assert r.entries_by_id(got) == [e.encode() for e in r.search(q)]
        r.set_low_latency(False)
        # the same id more than once, in the order asked, from any integer sequence
        first, last = 0, data.count(b'\n') - 1
        assert r.entries_by_id([last, first, last]) == [b'LASTENTRY', ref.entry(0), b'LASTENTRY']
        assert r.entries_by_id(np.array([first], dtype=np.int64)) == [ref.entry(0)]
        assert r.entries_by_id([]) == []
    finally:
        r.close()


@pytest.mark.parametrize('order', ['text', 'sa'])
def test_several_chunks_in_order(tmp_path, order):
    """Entries of one query in several chunks, an entry that holds the pattern twice: the ids come in the order of the
    packed entries, chunk-major."""
    rng = np.random.default_rng(12)
    data = b''.join(edge_text(np.random.default_rng(20 + k)) for k in range(5))
    p = make_index(tmp_path, 'multi', data, 24000)
    ref = IdRef.from_index(p)
    assert len(ref.chunks) >= 4 and sum(len(ch.text) for ch in ref.chunks) == len(data)
    r = pysubstringsearch.Reader(p, order=order)
    try:
        res = check(r, ref, EDGE_QUERIES + [filler(rng, 3) for _ in range(200)])
        twice = res.ids[sum(res.counts.tolist()[:EDGE_QUERIES.index(b'TWICE')]):][:res.counts[EDGE_QUERIES.index(b'TWICE')]]
        chunk_of = (twice >> np.uint64(32)).astype(np.int64)
        assert np.unique(chunk_of).size >= 2 and (np.diff(chunk_of) >= 0).all()      # several chunks, chunk-major
        assert r.entry_counts == ref.entry_counts()
        assert sum(r.entry_counts.values()) == data.count(b'\n')
    finally:
        r.close()


def test_line_numbers_of_an_indexed_file(tmp_path):
    rng = np.random.default_rng(13)
    words = ['alpha', 'beta', 'gamma', 'delta', 'omega', 'user=17', 'user=171', '']
    lines = [' '.join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(0, 6)))) for _ in range(6000)]
    lines[0] = 'the first line'
    lines[-1] = 'the last line'
    src = tmp_path / 'log.txt'
    src.write_text('\n'.join(lines) + '\n')
    p = str(tmp_path / 'log.idx')
    w = pysubstringsearch.Writer(p, 9000)
    w.add_entries_from_file_lines(str(src))
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert r.num_chunks >= 8
        assert sum(r.entry_counts.values()) == len(lines)
        for q in ['alpha', 'user=17', 'user=171', 'a b', 'the first line', 'the last line', 'line', '', 'beta gamma', 'zeta']:
            ids = r.search_ids(q)
            want = [i for i, ln in enumerate(lines) if q in ln]
            assert np.sort(r.entry_ordinals(ids)).tolist() == want, q
            assert sorted(r.entries_by_id(ids)) == sorted(lines[i].encode() for i in want)
        assert r.entry_ordinals([]).size == 0 and r.entry_ordinals([]).dtype == np.int64
        with pytest.raises(ValueError):
            r.entry_ordinals([(1 << 32) | r.entry_counts[1]])       # one past the last entry of chunk 1
    finally:
        r.close()
    shard = pysubstringsearch.Reader(p, shard=(1, 2))
    try:
        with pytest.raises(ValueError, match='chunk 0'):
            shard.entry_ordinals(shard.search_ids('alpha'))
    finally:
        shard.close()


def test_chunks_handed_over_on_the_device(search_env):
    """Text that does not end in a newline, one-entry chunks, and a chunk replaced after ids were served."""
    rng = np.random.default_rng(14)
    texts = [edge_text(rng, close=False), b'ONLYONE\n', b'NOEND', b'\n', b'x', edge_text(rng)]
    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = pysubstringsearch.Reader._from_handle(h)
    try:
        for t in texts[:3]:
            dt, ds = device_chunk(t)
            _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), len(t)))
        qs = EDGE_QUERIES + [b'ONLYONE', b'ONLY', b'NOEND', b'NOEN', b'D', b'x']
        ref = IdRef(texts[:3])
        assert ref.chunks[0].num_entries == texts[0].count(b'\n') + 1 and ref.chunks[2].num_entries == 1
        check(r, ref, qs)
        assert r.entry_counts == ref.entry_counts() == {0: texts[0].count(b'\n') + 1, 1: 1, 2: 1}
        assert r.entries_by_id([1 << 32, 2 << 32]) == [b'ONLYONE', b'NOEN']      # (no newline follows: the entry rule stops at n - 1)
        grown = r.residency['hbm_bytes']
        # chunks appended after ids were served get their tables on the next call
        for t in texts[3:]:
            dt, ds = device_chunk(t)
            _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), len(t)))
        ref = IdRef(texts)
        check(r, ref, qs)
        assert r.entry_counts == ref.entry_counts()
        assert r.residency['hbm_bytes'] > grown
        # a replaced chunk: same size (the allocation is reused) and another size; the new chunk's ids, not the old ones
        same = texts[0].replace(b'FIRSTENTRY', b'NEWFIRST\n\n').replace(b'LASTENTRY', b'NEW\nLAST\n')
        assert len(same) == len(texts[0]) and same.count(b'\n') != texts[0].count(b'\n')
        for at, new in ((0, same), (1, b'REPLACED one\nREPLACED two\n\nthree'), (5, b'short\n')):
            dt, ds = device_chunk(new)
            _ffi.check(_ffi.lib.pss_reader_set_chunk_device(h, at, dt.data_ptr(), ds.data_ptr(), len(new)))
            texts[at] = new
            ref = IdRef(texts)
            check(r, ref, qs + [b'NEWFIRST', b'NEW', b'LAST', b'REPLACED', b'three', b'thre', b'short'])
            assert r.entry_counts == ref.entry_counts()
    finally:
        r.close()


def test_batch_sizes(tmp_path, search_env):
    """No query, no hit, and more kept hits than the mid pipeline holds (65536): the general pipeline's buffers at size."""
    rng = np.random.default_rng(15)
    n = 1 << 20
    raw = np.frombuffer(FILLER, np.uint8)[rng.integers(0, len(FILLER), n)].copy()
    raw[rng.integers(0, n, n // 24)] = 0x0A
    raw[-1] = 0x0A
    data = raw.tobytes()
    p = make_index(tmp_path, 'big', data, 400000)
    ref = IdRef.from_index(p)
    assert len(ref.chunks) >= 3
    for order in ('text', 'sa'):
        r = pysubstringsearch.Reader(p, order=order)
        try:
            res = check(r, ref, [])
            assert res.ids.size == 0 and res.counts.size == 0
            res = check(r, ref, [b'MISS', b'\x01', b'zzzz'])
            assert res.ids.size == 0 and res.counts.tolist() == [0, 0, 0]
            heavy = [bytes([b]) for b in FILLER[:8]] + [b'ab', b'', b'\n', b'MISS']
            res = check(r, ref, heavy, texts=False)
            assert res.ids.size > 4 * 65536
        finally:
            r.close()


def test_placement(tmp_path, search_env):
    """Two parts on one device, a shard, a suffix array on the host tier: the same ids as the whole-file reader."""
    rng = np.random.default_rng(16)
    data = b''.join(edge_text(np.random.default_rng(30 + k)) for k in range(6))
    p = make_index(tmp_path, 'place', data, 24000)
    ref = IdRef.from_index(p)
    nchunks = len(ref.chunks)
    assert nchunks >= 5
    qs = EDGE_QUERIES + [filler(rng, 2) for _ in range(100)]
    whole = pysubstringsearch.Reader(p)
    try:
        base = check(whole, ref, qs)
        hbm = whole.residency['hbm_bytes'] - table_bytes(ref)
        chunk_of = (base.ids >> np.uint64(32)).astype(np.int64)
        query_of = np.repeat(np.arange(len(qs)), base.counts.astype(np.int64))
        # devices=[0, 0]: part-major inside a query; the ids of one file mean the same in every part
        multi = pysubstringsearch.Reader(p, devices=[0, 0])
        try:
            got = check(multi, ref, qs)
            assert got.counts.tolist() == base.counts.tolist()
            key = np.lexsort((np.arange(base.ids.size), chunk_of % 2, query_of))      # the whole reader's ids, part-major
            assert np.array_equal(got.ids, base.ids[key])
            assert multi.entry_counts == whole.entry_counts == ref.entry_counts()
            assert multi.entries_by_id(base.ids) == whole.entries_by_id(base.ids)
            assert multi.entry_ordinals(base.ids).tolist() == whole.entry_ordinals(base.ids).tolist()
            with pytest.raises(ValueError, match='has .* entries'):
                multi.entries_by_id([(1 << 32) | ref.chunks[1].num_entries])
            with pytest.raises(ValueError, match='does not hold chunk'):
                multi.entries_by_id([nchunks << 32])
        finally:
            multi.close()
        # shard (1, 2): the whole reader's ids of the odd chunks, in the same order
        shard = pysubstringsearch.Reader(p, shard=(1, 2))
        try:
            sref = IdRef.from_index(p, keep=lambda c: c % 2 == 1)
            got = check(shard, sref, qs)
            assert np.array_equal(got.ids, base.ids[chunk_of % 2 == 1])
            assert shard.entry_counts == {c: k for c, k in ref.entry_counts().items() if c % 2 == 1}
            with pytest.raises(ValueError, match='does not hold chunk 0'):
                shard.entries_by_id([0])                                            # chunk 0 lives in the other shard
            with pytest.raises(ValueError, match='has .* entries'):
                shard.entries_by_id([(1 << 32) | ref.chunks[1].num_entries])        # one past the last entry of chunk 1
            assert shard.entries_by_id([(1 << 32) | (ref.chunks[1].num_entries - 1)]) == [ref.chunks[1].entry(ref.chunks[1].num_entries - 1)]
            check(shard, sref, qs[:20])                                             # the reader still answers
        finally:
            shard.close()
    finally:
        whole.close()
    # one suffix array too many for the budget: it stays in pinned host memory, the line tables are in HBM all the same
    search_env(PSS_READER_HBM_BUDGET=hbm - 1, PSS_READER_AUTO_RESIDENCY=0)
    tier = pysubstringsearch.Reader(p)
    try:
        assert tier.residency['host_chunks'] >= 1
        got = check(tier, ref, qs)
        assert np.array_equal(got.ids, base.ids)
        assert tier.residency['host_chunks'] >= 1
    finally:
        tier.close()


def test_line_tables_are_built_on_demand(tmp_path):
    """A reader that never asks for ids holds nothing for them; the first ids call adds the tables, once."""
    rng = np.random.default_rng(17)
    data = b''.join(edge_text(np.random.default_rng(40 + k)) for k in range(4))
    p = make_index(tmp_path, 'lazy', data, 24000)
    ref = IdRef.from_index(p)
    qs = EDGE_QUERIES + [filler(rng, 2) for _ in range(50)]
    a, b = pysubstringsearch.Reader(p), pysubstringsearch.Reader(p)
    try:
        assert a.residency == b.residency
        before = a.search_batch_packed(qs)
        a.count_multiple_bytes(qs)
        a.search(qs[4].decode())
        assert a.residency == b.residency                      # searches and counts build nothing
        fresh = a.residency['hbm_bytes']
        check(a, ref, qs)
        grown = a.residency['hbm_bytes'] - fresh
        assert 0 < grown <= table_bytes(ref), (grown, table_bytes(ref))
        assert b.residency['hbm_bytes'] == fresh
        check(a, ref, qs[:10])
        assert a.entry_counts == ref.entry_counts()
        assert a.residency['hbm_bytes'] - fresh == grown      # built once
        after = a.search_batch_packed(qs)
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        # entry_counts alone builds them too
        assert b.entry_counts == ref.entry_counts()
        assert b.residency['hbm_bytes'] - fresh == grown
    finally:
        a.close()
        b.close()
