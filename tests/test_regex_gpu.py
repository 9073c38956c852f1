"""Regular-expression search (Reader.search_regex_ids_batch / search_regex_batch_packed / count_regex_bytes and the str
conveniences) against the brute-force reference of tests/regex_ref.py -- Python's re over every entry.  Every batch goes
through the check() of tests/search_harness.py with the REGEX / REGEX_ICASE kinds: ids, counts, packed text, routes and
`hits` are all held to the reference.
The cases: what the syntax means on a README-sized example; entry lengths around the 8-byte steps of the walk with the
match flush at either end, with and without `^` / `$`; chunk edges (device hand-over, an unterminated last entry); the walk
never crosses a newline; candidates that hold every literal and fail the expression; the two early exits; batches of 63 /
64 / 65 patterns with tables of different sizes; a table just under the state cap beside tiny ones; 0x00 and 0x80 .. 0xFF
in text and sets; fold; void patterns; placement; errors."""
import ctypes
import re

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, regex_escape, regex_info, regex_literals, regex_match
from tests import search_harness as H
from tests.regex_ref import REGEX, REGEX_ICASE, RegexRef
from tests.search_harness import device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu


def check(r, ref, patterns, fold=None, **kw):
    """patterns on reader r against ref, exact and under fold (fold=False / True: one of them).  Returns the exact IdResult."""
    res = None
    if fold is not True:
        res = H.check(REGEX, r, ref, list(patterns), **kw)
    if fold is not False:
        folded = H.check(REGEX_ICASE, r, ref, list(patterns), **kw)
        res = folded if res is None else res
    return res


def one_chunk(lines, closed=True):
    return H.one_chunk(RegexRef, lines, closed)


def texts_of(r, ids):
    return sorted(r.entries_by_id(ids))


# ---- 1. meaning ------------------------------------------------------------------------------------------------------------

def test_meaning():
    rng = np.random.default_rng(211)
    lines = [b'GET /api/v2/users/17 503', b'POST /api/v12/users/9 500', b'PUT /api/v2/users/17 503', b'GET /api/v2/users/x 503',
             b'GET /api/v2/users/17 505', b'user=bob_7@example.com', b'user=amy@example.org', b'user=@example.com', b'user=al@example.net',
             b'2024-01-02 db timeout after 12 ms', b'2024-01-02 db timeout after 12 ms!', b'x 2024-01-02 db timeout after 1 ms',
             b'24-01-02 db timeout after 12 ms', b'abc', b'abbbc', b'ac', b'a.c', b'a|c', b'Abc', b'']
    lines += [filler(rng, int(rng.integers(0, 30))).replace(b'a', b'p') for _ in range(200)]       # (no `a`: the answers below are exact)
    r, ref, data = one_chunk(lines)
    patterns = [rb'(GET|POST) /api/v[0-9]+/users/\d+ 50[0-4]', rb'user=\w+@example\.(com|org)', rb'^\d{4}-\d\d-\d\d .* timeout after \d+ ms$',
                rb'ab+c', rb'ab*c', rb'^ab?c$', rb'a\.c', rb'a.c', rb'a\|c', rb'^a(?:bc|c)$', rb'a[^b]c', rb'ab{2,3}c', rb'(ab){1}b{2}c$', rb'users/(17|9) ']
    try:
        res = per_pattern(check(r, ref, patterns, fold=False))
        t = lambda i: texts_of(r, res[i])
        assert t(0) == [b'GET /api/v2/users/17 503', b'POST /api/v12/users/9 500']
        assert t(1) == [b'user=amy@example.org', b'user=bob_7@example.com']
        assert t(2) == [b'2024-01-02 db timeout after 12 ms']
        assert t(3) == [b'abbbc', b'abc'] and t(4) == [b'abbbc', b'abc', b'ac'] and t(5) == [b'abc', b'ac']
        assert t(6) == [b'a.c'] and t(7) == [b'a.c', b'abc', b'a|c'] and t(8) == [b'a|c'] and t(9) == [b'abc', b'ac']
        assert t(10) == [b'a.c', b'a|c'] and t(11) == [b'abbbc'] and t(12) == [b'abbbc'] and len(t(13)) == 4
        check(r, ref, patterns, fold=True)
        assert sorted(r.search_regex('^ABC$', icase=True)) == ['Abc', 'abc'] and r.search_regex('^ABC$') == []
        assert r.count_regex('ab+c') == 2 and r.count_regex(b'AB+C', icase=True) == 3
    finally:
        r.close()


# ---- 2. the 8-byte steps ---------------------------------------------------------------------------------------------------

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def test_entry_lengths_around_the_load_width():
    """Entries of every length around the 8-byte step with the marker Q flush at the first and at the last byte, a short entry
    in front moving the start against the 8-byte grid; patterns that pin Q to either end with and without ^ / $, and counted
    classes that take the whole entry exactly."""
    rng = np.random.default_rng(212)
    lines, patterns = [], []
    for n in LENGTHS:
        for lead in range(3):
            lines += [filler(rng, lead), b'Q' + filler(rng, n - 1), filler(rng, n - 1) + b'Q', filler(rng, n) + b'Q' + filler(rng, n)]
        patterns += [b'^Q[a-p]{%d}$' % (n - 1), b'^[a-p]{%d}Q$' % (n - 1), b'^Q.{%d}$' % (n - 1), b'^.{%d}Q$' % (n - 1), b'^Q[a-p]{%d}' % (n - 1),
                     b'[a-p]{%d}Q$' % (n - 1), b'Q[a-p]{%d}' % n, b'[a-p]{%d}Q' % n, b'^[a-p]{%d}Q[a-p]{%d}$' % (n, n)]
    patterns += [b'^Q', b'Q$', b'^Q$', b'^Q[a-p]*$', b'^[a-p]*Q$', b'Q']
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, patterns)
        assert (res.counts > 0).all()
    finally:
        r.close()


# ---- 3. chunk edges ----------------------------------------------------------------------------------------------------------

def test_chunk_edges_handed_over_on_the_device():
    """The first entry of a chunk, and an unterminated last entry whose last byte takes part in the match."""
    texts = [b'ab\nxx\nab', b'b', b'q\x00\nqa\nzq', b'a', b'\n', b'cd\nc', b'ab\n\nb7\n', b'abcdefgh12345678Q']
    patterns = [b'^ab$', b'^a', b'b$', b'^b$', b'ab', b'^q.$', b'^q\\x00', b'q$', b'^c$', b'^cd', b'b\\d$', b'^.b$', b'^[a-h]{8}\\d{8}Q$', b'8Q$', b'^a.*Q$',
                b'^a.{15}$', b'^a.{16}$']
    r, ref = device_reader(texts), RegexRef(texts)
    try:
        res = per_pattern(check(r, ref, patterns))
        assert res[0].size == 3 and res[3].size == 1 and res[12].size == 1 and res[15].size == 0 and res[16].size == 1
    finally:
        r.close()
    r, ref, data = one_chunk([b'xa', b'ab', b'Qa' + b'c' * 14], closed=False)
    try:
        res = per_pattern(check(r, ref, [b'^xa$', b'a$', b'^Q.*c$', b'^Qac{14}$', b'^Qac{13}$']))
        assert res[0].size == 1 and res[2].size == 1 and res[3].size == 1 and res[4].size == 0
    finally:
        r.close()


# ---- 4. the walk stays inside the entry ------------------------------------------------------------------------------------

def test_the_walk_never_crosses_the_newline():
    r, ref, data = one_chunk([b'ab', b'cd', b'ab cd', b'ab', b'', b'cd'])
    try:
        res = per_pattern(check(r, ref, [rb'ab\scd', b'ab[^x]cd', b'ab.?cd', rb'ab\n?cd', b'ab[^x]*cd', rb'ab\Wcd', b'^cd$', b'ab$']))
        assert all(texts_of(r, res[i]) == [b'ab cd'] for i in (0, 1, 2, 4, 5)) and res[3].size == 0
    finally:
        r.close()


# ---- 5. literals present, expression failing ------------------------------------------------------------------------------

def test_candidates_that_hold_every_literal_and_fail():
    rng = np.random.default_rng(215)
    lines = [b'alpha 12 beta', b'alpha x beta', b'beta 12 alpha', b'alpha 1234 beta', b'alphabeta', b'alpha 12 bet', b'beta alpha 7 beta']
    lines += [filler(rng, int(rng.integers(0, 20))) for _ in range(100)]
    r, ref, data = one_chunk(lines)
    patterns = [rb'alpha \d+ beta', rb'alpha \d{2} beta', rb'alpha.*beta', rb'beta.*alpha', rb'^alpha \d+ beta$', rb'alpha (\d\d)+ beta']
    try:
        assert regex_literals(patterns[0]) == [b'alpha ', b' beta']
        res = per_pattern(check(r, ref, patterns))
        assert texts_of(r, res[0]) == [b'alpha 12 beta', b'alpha 1234 beta', b'beta alpha 7 beta'] and texts_of(r, res[1]) == [b'alpha 12 beta']
        assert texts_of(r, res[3]) == [b'beta 12 alpha', b'beta alpha 7 beta']         # the wrong order is dropped from [2], kept here
        assert b'beta 12 alpha' not in texts_of(r, res[2])
    finally:
        r.close()


# ---- 6. early exits ------------------------------------------------------------------------------------------------------------

def test_dead_state_and_sink_in_the_first_byte():
    rng = np.random.default_rng(216)
    lines = [b'Q' + filler(rng, 70), b'a' + filler(rng, 30) + b'Q' + filler(rng, 40), filler(rng, 64) + b'Q', b'Q', b'aQ']
    r, ref, data = one_chunk(lines)
    try:
        info = regex_info(b'^Q')
        assert info['sink'] >= info['first_accept'] and regex_info(b'^Q$')['sink'] == 0
        res = per_pattern(check(r, ref, [b'^Q', b'^Q.*', b'^[^a]*Q', b'Q', b'^Q$', b'^.Q']))
        assert res[0].size == 2 and res[3].size == 5 and res[4].size == 1 and res[5].size == 1
    finally:
        r.close()


# ---- 7. many patterns, tables of different sizes ------------------------------------------------------------------------------

def edge_regexes(groups):
    """The triples of search_harness.edge_groups as patterns of two literals with gaps of different kinds between them, so
    that the tables of one batch differ in size; every other one anchored at both ends."""
    gaps = (b'.*', b'[a-pA-P]*', b'.{0,3}.*', b'(?:[a-p]|[A-P]){0,9}.*', b'[^Q]*')
    out = []
    for i, (a, b, _) in enumerate(groups):
        body = regex_escape(a) + gaps[i % len(gaps)] + regex_escape(b)
        out.append(body if i % 2 else b'^' + body + b'$')
    return out


@pytest.mark.parametrize('kind', [REGEX, REGEX_ICASE], ids=lambda kind: kind.name)
def test_rows_and_literal_bytes_around_a_multiple_of_64(kind):
    H.layout_edges(kind, edge_regexes, min_ids=63)


def test_a_table_just_under_the_state_cap_beside_tiny_ones():
    rng = np.random.default_rng(218)
    big = b'x(a|b)*a(a|b){11}'             # the last of its family that compiles (tests/test_regex_host.py::test_state_cap)
    assert 2048 < regex_info(big)['states'] <= 4096
    with pytest.raises(ValueError, match='too complex'):
        regex_info(b'x(a|b)*a(a|b){12}')
    big_end = b'x(a|b)*a(a|b){10}$'        # under `$` the accepting subsets stay apart: the last of ITS family that compiles
    assert 2048 < regex_info(big_end)['states'] <= 4096 and regex_info(big_end)['sink'] == 0
    lines = [b'x' + bytes(rng.choice(np.frombuffer(b'ab', np.uint8), int(n))) for n in rng.integers(8, 40, 120)] + [b'xab', b'abab', b'x']
    r, ref, data = one_chunk(lines)
    try:
        res = per_pattern(check(r, ref, [b'xa', big, b'^x$', big_end, b'xb+a'], fold=False))
        assert 0 < res[1].size < 120 and 0 < res[3].size < res[1].size
    finally:
        r.close()


# ---- 8. bytes, fold, voids ---------------------------------------------------------------------------------------------------

def test_every_byte_in_text_and_sets():
    lines = [b'k' + bytes([b]) + b'z' for b in range(256) if b != 0x0A] + [b'k\x00\x00z', b'kz']
    r, ref, data = one_chunk(lines)
    try:
        res = per_pattern(check(r, ref, [rb'k[\x00-\x1f]z', rb'k[\x80-\xff]z', rb'k[^\x00]z', rb'k\x00+z', rb'k\0z', b'k\xc3z', rb'k[\xc0-\xc5]z', rb'k\Wz',
                                         rb'k[^\x80-\xff]z', rb'k.z', rb'k[\d\x00]z']))
        assert res[0].size == 31 and res[1].size == 128 and res[2].size == 254 and res[3].size == 2 and res[5].size == 1 and res[9].size == 255
    finally:
        r.close()


def test_fold(search_env):
    lines = [b'Hello World', b'hello world', b'HELLO WORLD', b'hellO xorld', b'xAy', b'xay', b'xby', b'xBy', b'x@y', b'x`y', b'x[y', b'x{y', b'k\xc1z', b'k\xe1z']
    patterns = [b'hello w', b'HELLO [^x]orld', b'x[^a]y', b'x[^A]y', b'x[a-b]y', b'x[@-A]y', b'x[`-a]y', b'x[Z-a]y', b'k\xc1z', rb'^x\wy$', rb'x[\W]y', b'h(e|E)llo']
    r, ref, data = one_chunk(lines)
    try:
        for letters in (1, 3):
            search_env(PSS_ICASE_SEED_LETTERS=letters)
            res = per_pattern(check(r, ref, patterns, fold=True))
        assert res[0].size == 3 and texts_of(r, res[2]) == sorted([b'xby', b'xBy', b'x@y', b'x`y', b'x[y', b'x{y']) and res[8].size == 1
        assert np.array_equal(res[2], res[3])
        check(r, ref, patterns, fold=False)
    finally:
        search_env(PSS_ICASE_SEED_LETTERS=None)
        r.close()


def test_void_patterns_beside_live_ones():
    r, ref, data = one_chunk([b'ab', b'cd', b'abcd'])
    try:
        res = per_pattern(check(r, ref, [b'ab', rb'b\ncd', b'cd', rb'ab\x0a', b'b\nc.*', b'^abcd$']))
        assert res[1].size == 0 and res[3].size == 0 and res[4].size == 0 and res[0].size == 2 and res[5].size == 1
        void = r.search_regex_ids_batch([rb'b\nc'])
        assert void.ids.size == 0 and r.last_stats()['hits'] == 0
    finally:
        r.close()


# ---- 9. placement ------------------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(220)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = RegexRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'a.b', b'b[a-d]a', b'^a.*b$', rb'^HEAD\d[0-4]\d ', b'HEAD.*a.+b', b'p[^p]', b'ab.*(cd|dc)', b'MISS.a', b'^e.', b'.e$', rb'HEAD\d+ [a-p]{6}$',
                b'(ab)+c', b'a{2,}b']
    for kind in (REGEX, REGEX_ICASE):
        assert H.placement(kind, p, patterns, search_env, ref=ref).ids.size > 100


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------

def test_errors():
    rng = np.random.default_rng(221)
    r, ref, data = one_chunk([filler(rng, int(rng.integers(0, 10))) for _ in range(100)] + [b'ab', b'a1b'])
    try:
        for call in (r.search_regex_batch_packed, r.search_regex_ids_batch, r.count_regex_bytes):
            for bad, what in (([b'ab', b'a*?'], 'pattern 1: a lazy quantifier'), ([rb'\d+'], 'without a required literal'), ([b'a|b'], 'required literal'),
                              ([b'(a'], 'without its \\)'), ([b''], 'empty pattern'), ([b'x(a|b)*a(a|b){13}'], 'too complex'), ([b'a{3000}'], 'too complex'),
                              ([b'^a|b'], 'bare alternation')):
                for fold in (False, True):
                    with pytest.raises(ValueError, match=what):
                        call(bad, icase=fold)
            with pytest.raises(TypeError):
                call(b'ab')
            with pytest.raises(TypeError):
                call([b'ab'], icase=1)
            with pytest.raises(TypeError):
                call([7])
        h = r._handle()
        blob, offs = b'aba*?', np.array([0, 2, 5], dtype=np.uint64)
        for fn in (_ffi.lib.pss_reader_search_regex_batch, _ffi.lib.pss_reader_search_regex_ids_batch):
            out = ctypes.c_void_p()
            assert fn(h, blob, offs.ctypes.data, 2, 0, ctypes.byref(out)) == _ffi.PSS_EINVAL
            assert not out.value and 'pattern 1' in _ffi.last_error()
            assert fn(h, blob, offs.ctypes.data, 1, 2, ctypes.byref(out)) == _ffi.PSS_EINVAL and 'flags' in _ffi.last_error()
            assert fn(h, blob, offs.ctypes.data, 1, 0, None) == _ffi.PSS_EINVAL
        counts = np.full(4, 7, dtype=np.uint64)
        assert _ffi.lib.pss_reader_count_regex_batch(h, blob, offs.ctypes.data, 2, 0, counts.ctypes.data) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4
        out = ctypes.c_void_p()                             # ... and the good batch goes through the same call; the reader still answers
        assert _ffi.lib.pss_reader_search_regex_batch(h, blob, offs.ctypes.data, 1, 0, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) >= 1
        _ffi.lib.pss_result_free(out)
        assert r.search_regex_ids_batch([]).ids.size == 0
        r.set_result_order('sa')
        check(r, ref, [b'a.b', rb'a\d?b'])
    finally:
        r.close()


def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    w.add_entry('some short string')
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        one = ['some short string']
        assert r.search_regex(r'some\s+sh[a-o]rt') == r.search_regex(r'^some.*string$') == r.search_regex('SOME (long|short)', icase=True) == one
        assert r.search_regex('some long') == [] and r.search_regex('SOME') == [] and r.search_regex('^short') == []
        assert r.count_regex('s.r') == 1 and r.count_regex('S.R', icase=True) == 1 and r.count_regex('s.r$') == 0
        assert regex_match(b'some\\s+sh', b'some short string') and re.search(regex_escape(b'a.b*[c]'), b'xa.b*[c]')
    finally:
        r.close()
