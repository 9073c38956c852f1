"""Match spans on the engine (include/pss.h, pss_reader_match_spans): Reader.match_spans_batch row by row
against the brute-force reference of tests/span_ref.py, on one-chunk and few-chunk readers whose texts stay under 10 KB.
Entry shapes, wave steps and lane edges, ties, newlines, case folding, budgets and pattern lengths, batch shapes, reader
placements, and that the calls beside it answer as before."""
import numpy as np
import pytest

import pysubstringsearch
from tests.search_harness import device_reader, make_index, one_chunk
from tests.span_ref import NONE, SpanRef

pytestmark = pytest.mark.gpu

FLAGS = [(False, False), (False, True), (True, False), (True, True)]       # (edits, icase)


def check(r, ref, ids, counts, patterns, k, edits=False, icase=False):
    """One batch on reader r against ref, row by row; returns the rows."""
    got = r.match_spans_batch(ids, counts, patterns, k, edits, icase=icase)
    want = ref.spans(ids, counts, patterns, k, edits, icase)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (len(ids), 3)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        q = int(np.searchsorted(np.cumsum(counts), i, side='right'))
        raise AssertionError(('row', i, 'entry', ref.true_entry(ids[i])[:80], 'pattern', patterns[q][:40], 'k', k, 'edits', edits, 'icase', icase,
                              'got', got[i].tolist(), 'want', want[i].tolist(), 'rows wrong', int(bad.size)))
    return got


def every(r, ref, patterns, k, flags=FLAGS):
    """Every entry of the reader against every pattern, under every combination of flags; {(edits, icase): rows}."""
    ids = ref.all_ids()
    out = {}
    for edits, icase in flags:
        out[edits, icase] = check(r, ref, np.tile(ids, len(patterns)), [ids.size] * len(patterns), patterns, k, edits, icase)
    return out


def rows_of(got, n, q):
    """The rows of pattern q of a batch of every(): one per entry."""
    return got[q * n:(q + 1) * n].tolist()


# ---- entry shape -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_entry_lengths_around_the_pattern(k):
    p = b'abcdefgh'
    L = len(p)
    # the chunk's first entry, entries of L - k - 1, L - k, L, L + k bytes cut from the pattern, empty entries (two
    # newlines in a row), and an unterminated last entry whose best match ends flush with n
    lines = [p, p[:L - k - 1], p[:L - k], p[k:], b'', b'', b'x' * k + p, p + b'y' * k, b'', b'zz' + p]
    r, ref, data = one_chunk(SpanRef, lines, closed=False)
    try:
        assert data.endswith(p) and b'\n\n\n' in data
        got = every(r, ref, [p], k)
        n = len(lines)
        for (edits, icase), rows in got.items():
            assert rows[0].tolist() == [0, L, 0] and rows[n - 1].tolist() == [2, L, 0]
            assert rows[4].tolist() == list(NONE) and rows[8].tolist() == list(NONE)
            assert rows[1].tolist() == list(NONE)                          # L - k - 1 bytes: out of reach of either budget
            assert rows[2].tolist() == ([0, L - k, k] if edits or k == 0 else list(NONE))
            if not edits:
                assert (rows[rows[:, 2] >= 0][:, 1] == L).all()
    finally:
        r.close()


def test_a_pattern_ending_in_zero_bytes_at_the_chunks_end():
    """Behind n stands zero padding: it is no text, for a window and for the band's walk alike."""
    lines = [b'ab\x00\x00', b'xxab\x00', b'ab']
    r, ref, data = one_chunk(SpanRef, lines, closed=False)
    try:
        pats = [b'ab\x00\x00', b'ab\x00', b'b\x00\x00\x00', b'xab\x00\x00']
        got = every(r, ref, pats, [1, 0, 2, 1])
        n = len(lines)
        assert rows_of(got[False, False], n, 0) == [[0, 4, 0], list(NONE), list(NONE)]      # `xab\0` and `ab` + padding: no
        assert rows_of(got[False, False], n, 1) == [[0, 3, 0], [2, 3, 0], list(NONE)]
        assert rows_of(got[True, False], n, 1)[2] == list(NONE) and rows_of(got[True, False], n, 0)[2] == list(NONE)
        assert rows_of(got[True, False], n, 2)[2] == list(NONE)
        assert rows_of(got[True, False], n, 0)[1] == [2, 3, 1]                              # `ab\0`: one deletion, the entry ends there
    finally:
        r.close()
    r, ref, data = one_chunk(SpanRef, [b'q', b'xab\x00'], closed=False)                     # ... and the same flush with n
    try:
        got = every(r, ref, [b'ab\x00\x00', b'ab\x00'], [1, 0])
        assert rows_of(got[False, False], 2, 0)[1] == list(NONE) and rows_of(got[True, False], 2, 0)[1] == [1, 3, 1]
        assert rows_of(got[False, False], 2, 1)[1] == [1, 3, 0]
    finally:
        r.close()


# ---- wave steps and lane edges -----------------------------------------------------------------------------------------------

def planted(length, at, word, fill=b'x'):
    assert at + len(word) <= length
    return fill * at + word + fill * (length - at - len(word))


def test_entry_lengths_and_match_starts_around_the_wave():
    p, near = b'needle', b'neXdle'
    L = len(p)
    lines, where = [], []
    for length in (63, 64, 65, 127, 128, 129):
        for at in (0, 63, 64, 65, 127, 128, length - L):
            if 0 <= at <= length - L:
                lines.append(planted(length, at, p if len(lines) % 2 else near))
                where.append(at)
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        assert len(data) < 10000
        got = every(r, ref, [p, p.upper()], [1, 2])
        assert got[False, False][:len(lines), 0].tolist() == where and got[True, False][:len(lines), 0].tolist() == where
        assert got[True, True][len(lines):, 0].tolist() == where and (got[False, False][len(lines):, 2] == -1).all()
        assert sorted(set(got[False, False][:len(lines), 2].tolist())) == [0, 1]
    finally:
        r.close()


def test_a_long_entry_and_the_order_of_the_steps():
    a, b, c, d, e = b'alpha1', b'bravo2', b'charl3', b'delta4', b'echo55'
    n = 5000
    body = bytearray(b'.' * n)

    def put(at, word):
        body[at:at + len(word)] = word

    put(0, a)                   # start 0 ...
    put(n - 6, b)               # ... and the last possible start
    put(10, b'chXrl3')          # the same distance in two different steps: the earlier start wins
    put(700, b'chYrl3')
    put(20, b'dXltY4')          # a worse match in step 0, a better one in step 2
    put(150, b'dZlta4')
    put(100, e)                 # distance 0 in step 1, and once more later
    put(3000, e)
    put(40, b'echo5Q')          # (and a worse one in front of it, in step 0)
    r, ref, data = one_chunk(SpanRef, [b'short', bytes(body), b'tail'])
    try:
        assert len(data) < 10000
        got = every(r, ref, [a, b, c, d, e], [1, 1, 1, 2, 1])
        for flags, rows in got.items():
            assert [rows_of(rows, 3, q)[1] for q in range(5)] == [[0, 6, 0], [n - 6, 6, 0], [10, 6, 1], [150, 6, 1], [100, 6, 0]], flags
    finally:
        r.close()


# ---- ties --------------------------------------------------------------------------------------------------------------------

def test_ties():
    lines = [b'passw0rd password', b'passw0rd passw1rd', b'zbcd', b'abxc', b'abcabc', b'xxabcdxxabcdxx', b'aXcd abXd', b'bcd', b'abcd' * 20]
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        pats = [b'password', b'abcd', b'abc']
        got = every(r, ref, pats, 1)
        n = len(lines)
        plain, edit = got[False, False], got[True, False]
        assert rows_of(plain, n, 0)[:2] == [[9, 8, 0], [0, 8, 1]] and rows_of(edit, n, 0)[:2] == [[9, 8, 0], [0, 8, 1]]
        assert rows_of(edit, n, 1)[2] == [0, 4, 1]          # `zbcd` for `abcd`: the longest at start 0, not `bcd`
        assert rows_of(edit, n, 2)[3] == [0, 4, 1]          # `abxc` for `abc`: the longest, not `ab`
        assert rows_of(plain, n, 2)[4] == [0, 3, 0] and rows_of(plain, n, 1)[5] == [2, 4, 0]      # equal distance at two starts
        assert rows_of(plain, n, 1)[6] == [0, 4, 1] and rows_of(edit, n, 1)[7] == [0, 3, 1]
        for q, p in enumerate(pats):                        # without edits the length is the pattern's
            for rows in (got[False, False], got[False, True]):
                sub = np.array(rows_of(rows, n, q))
                assert (sub[sub[:, 2] >= 0][:, 1] == len(p)).all() and (sub[sub[:, 2] < 0][:, 1] == 0).all()
        assert len({tuple(x[1:]) for x in rows_of(edit, n, 1) if x[2] >= 0}) >= 3                 # several lengths under edits
    finally:
        r.close()


# ---- newlines ----------------------------------------------------------------------------------------------------------------

def test_nothing_reaches_over_a_newline():
    lines = [b'abc', b'def', b'xabc', b'defx', b'ab', b'cdef', b'abcdef']
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        pats = [b'abcdef', b'abcXdef', b'abc\ndef', b'cdef', b'bc\n']
        got = every(r, ref, pats, [1, 1, 1, 1, 2])
        n = len(lines)
        for flags, rows in got.items():
            assert [x[2] for x in rows_of(rows, n, 0)] == [-1] * 6 + [0], flags               # `abc` + `def` next door is no match
            assert rows_of(rows, n, 2) == [list(NONE)] * n and rows_of(rows, n, 4) == [list(NONE)] * n      # a pattern with a newline
        assert [x[2] for x in rows_of(got[False, False], n, 1)] == [-1] * n                   # the newline is no wild byte
        assert [x[2] for x in rows_of(got[True, False], n, 1)] == [-1] * 6 + [1]
        assert rows_of(got[True, False], n, 3)[:2] == [list(NONE), [0, 3, 1]]                  # `def` for `cdef`; `c` + newline + `def` is not
    finally:
        r.close()


# ---- case folding -------------------------------------------------------------------------------------------------------------

def test_case_folding_folds_ascii_letters_only():
    lines = [b'@`[{', b'`@{[', b'\xc9t\xe9', b'\xe9T\xc9', b'PassWord', b'password', b'PASSW0RD', b'\x00aA\x80\xff', b'\x00Aa\x80\xff',
             b'abcdefghijklmnopqrstuvwxyz', b'Zz\x00\x00zZ', b'\xc1\xe1aA']
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        pats = [b'@`[{', b'\xc9t\xe9', b'pAsSwOrD', b'\x00Aa\x80\xff', b'MNOPQRST', b'zz\x00\x00ZZ', b'\xe1\xc1Aa']
        got = every(r, ref, pats, [0, 0, 1, 0, 0, 1, 2])
        n = len(lines)
        fold, plain = got[False, True], got[False, False]
        assert [x[2] for x in rows_of(fold, n, 0)[:2]] == [0, -1]                                      # `@` / '`', `[` / `{` do not fold
        assert [x[2] for x in rows_of(fold, n, 1)[2:4]] == [0, -1]                                     # nor 0xC9 / 0xE9
        assert [x[2] for x in rows_of(fold, n, 2)[4:7]] == [0, 0, 1] and [x[2] for x in rows_of(plain, n, 2)[4:7]] == [-1, -1, -1]
        assert [x[2] for x in rows_of(fold, n, 3)[7:9]] == [0, 0] and [x[2] for x in rows_of(plain, n, 3)[7:9]] == [-1, 0]
        assert rows_of(fold, n, 4)[9] == [12, 8, 0] and rows_of(plain, n, 4)[9] == list(NONE)           # [a-z] text, upper-case pattern
        assert rows_of(fold, n, 5)[10] == [0, 6, 0] and rows_of(fold, n, 6)[11] == [0, 4, 2] and rows_of(got[True, True], n, 6)[11] == [1, 3, 1]
    finally:
        r.close()


# ---- budgets and pattern length ------------------------------------------------------------------------------------------------

def test_budgets_per_pattern_and_pattern_lengths():
    rng = np.random.default_rng(2030)
    long = bytes(rng.integers(0x61, 0x67, 200, dtype=np.uint8))
    hurt = bytearray(long)
    hurt[17] ^= 1
    del hurt[120]
    hurt.insert(180, 0x7A)
    lines = [b'a', b'ab', b'abc', b'abcd', b'b', b'xb', b'bcd', b'', b'pre' + long + b'post', bytes(hurt) + b'!', long[:199], long[1:], b'abXd']
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        pats = [b'a', b'ab', b'abc', b'abcd', long, long, b'abcd', b'abcd']         # the shortest legal pattern of each budget, and 200 bytes
        ks = [0, 1, 2, 3, 0, 3, 0, 1]
        got = every(r, ref, pats, ks)
        n = len(lines)
        assert rows_of(got[False, False], n, 4)[8] == [3, 200, 0] and rows_of(got[False, False], n, 5)[9] == list(NONE)
        assert rows_of(got[True, False], n, 5)[9] == [0, 200, 3] and rows_of(got[True, False], n, 5)[10] == [0, 199, 1]
        assert rows_of(got[False, False], n, 6)[12] == list(NONE) and rows_of(got[False, False], n, 7)[12] == [0, 4, 1]
        assert rows_of(got[True, False], n, 3)[4] == [0, 1, 3]                      # one byte left of `abcd` at k = 3
    finally:
        r.close()


# ---- batch shape ---------------------------------------------------------------------------------------------------------------

def test_batch_shapes():
    texts = [b'error one\nwarning\nerrr two\n', b'nothing\nan eror\n', b'ERROR three\n\nterror']
    r, ref = device_reader(texts), SpanRef(texts)
    try:
        ids = ref.all_ids()
        assert ids.size == 8 and np.unique(ids >> np.uint64(32)).size == 3
        mixed = np.array([ids[7], ids[0], ids[3], ids[0], ids[5], ids[2], ids[7], ids[7], ids[4], ids[1], ids[6]], dtype=np.uint64)
        for edits, icase in FLAGS:
            # ids of three chunks interleaved and repeated; the same ids under two patterns; a pattern with zero rows
            got = check(r, ref, np.concatenate([mixed, mixed[::-1], ids[:2]]), [mixed.size, 0, mixed.size, 2],
                        [b'error', b'absent', b'eror', b'warnings'], [1, 0, 1, 2], edits, icase)
            assert np.array_equal(got[1], got[3]) and np.array_equal(got[0], got[6]) and (got[:, 2] >= 0).sum() >= 8
            # an empty batch, and patterns without rows
            for none in (r.match_spans_batch([], [], [], 1, edits, icase=icase), r.match_spans_batch([], [0, 0], [b'ab', b'c'], [1, 0], edits, icase=icase),
                         r.match_spans(np.zeros(0, dtype=np.uint64), b'error', 1, edits, icase=icase)):
                assert none.shape == (0, 3) and none.dtype == np.int32
            # the convenience form: one pattern, bytes or str, and any integer sequence of ids
            one = r.match_spans(mixed, b'error', 1, edits, icase=icase)
            assert np.array_equal(one, got[:mixed.size]) and np.array_equal(r.match_spans(mixed.tolist(), 'error', 1, edits, icase=icase), one)
            assert np.array_equal(r.match_spans(mixed.astype(np.int64), b'error', edits=edits, icase=icase), one)
        found = r.search_near_ids_batch([b'error', b'eror'], 1, edits=True, icase=True)
        got = check(r, ref, found.ids, found.counts, [b'error', b'eror'], 1, True, True)              # an IdResult's two fields as they come
        assert (got[:, 2] >= 0).all() and found.ids.size >= 8
        for bad in ([1 << 40], [ids[0], (2 << 32) | 3], [3]):
            with pytest.raises(ValueError, match='entry id'):
                r.match_spans(np.array(bad, dtype=np.uint64), b'error')
    finally:
        r.close()


# ---- readers -------------------------------------------------------------------------------------------------------------------

def test_placements_give_the_same_rows(tmp_path):
    rng = np.random.default_rng(2040)
    words = [b'error', b'eror', b'ERROR', b'terror', b'mirror', b'arrow', b'err', b'', b'warning: errr', b'x' * 70 + b'errorr']
    lines = [b' '.join(words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(1, 4)))) for _ in range(160)]
    data = b'\n'.join(lines) + b'\n'
    assert len(data) < 10000
    p = make_index(tmp_path, 'spans', data, 1200)
    ref = SpanRef.from_index(p)
    assert len(ref.chunks) >= 3
    ids = ref.all_ids()
    pick = ids[rng.permutation(ids.size)[:120]]
    pats, ks = [b'error', b'Mirror'], [1, 2]
    args = (np.tile(pick, 2), [pick.size, pick.size], pats, ks)
    Reader = pysubstringsearch.Reader
    whole = Reader(p)
    try:
        base = {f: check(whole, ref, *args, *f) for f in FLAGS}
        assert all((b[:, 2] >= 0).sum() > 20 and (b[:, 2] < 0).sum() > 20 for b in base.values())
    finally:
        whole.close()
    multi = Reader(p, devices=[0, 0])
    try:
        for f in FLAGS:
            assert np.array_equal(check(multi, ref, *args, *f), base[f])
        with pytest.raises(ValueError, match='does not hold chunk'):
            multi.match_spans(np.array([len(ref.chunks) << 32], dtype=np.uint64), b'error')
    finally:
        multi.close()
    for i in (0, 1):
        shard = Reader(p, shard=(i, 2))
        try:
            held = (np.tile(pick, 2) >> np.uint64(32)) % np.uint64(2) == i
            mine = pick[(pick >> np.uint64(32)) % np.uint64(2) == i]
            sref = SpanRef.from_index(p, keep=lambda c: c % 2 == i)
            for f in FLAGS:
                got = check(shard, sref, np.tile(mine, 2), [mine.size, mine.size], pats, ks, *f)
                assert np.array_equal(got, base[f][held])
            other = pick[(pick >> np.uint64(32)) % np.uint64(2) != i]
            assert mine.size and other.size
            with pytest.raises(ValueError, match='does not hold chunk'):                    # an id of a chunk the shard lacks
                shard.match_spans(np.concatenate([mine[:3], other[:1]]), b'error')
        finally:
            shard.close()


# ---- unchanged behaviour ---------------------------------------------------------------------------------------------------------

def test_the_calls_beside_it_answer_as_before():
    lines = [b'error one', b'warning', b'errr two', b'', b'ERROR three', b'an eror', b'terror']
    r, ref, data = one_chunk(SpanRef, lines)
    try:
        pats, ks = [b'error', b'warming'], [1, 2]
        before = {f: r.search_near_ids_batch(pats, ks, edits=f[0], icase=f[1]) for f in FLAGS}
        text = r.entries_by_id(ref.all_ids())
        for f in FLAGS:
            stats = r.last_stats()
            got = check(r, ref, before[f].ids, before[f].counts, pats, ks, *f)
            assert (got[:, 2] >= 0).all()
            every(r, ref, pats, ks, [f])
            assert r.last_stats() == stats                                                  # pss_reader_last_stats is left as it was
            after = r.search_near_ids_batch(pats, ks, edits=f[0], icase=f[1])
            assert np.array_equal(after.ids, before[f].ids) and np.array_equal(after.counts, before[f].counts)
            assert r.entries_by_id(ref.all_ids()) == text
        assert text == [ref.entry(i) for i in ref.all_ids().tolist()]
    finally:
        r.close()
