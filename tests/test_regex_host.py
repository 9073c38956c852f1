"""The host side of the regular-expression search (include/pss.h, pss_regex_compile; csrc/regex_compile.h): the parser and
what it refuses, the host matcher against Python's re on the seeded pairs of tests/regex_fuzz_cases.py, the required
literals, the two caps, the C entry points without a reader, the stubs, and the compiler alone under sanitizers
(tests/native/regex_compile.cpp).  CPU only."""
import ctypes
import inspect
import os
import pathlib
import re
import subprocess

import numpy as np
import pytest

import pysubstringsearch_amd as P
from pysubstringsearch_amd import _ffi, regex_escape, regex_info, regex_literals, regex_match
from tests.regex_fuzz_cases import SEEDS, make_regex_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (pattern, strings it matches, strings it does not)
PARSER = [
    (rb'ab', [b'ab', b'xaby'], [b'a', b'ba', b'']),
    (rb'a.c', [b'abc', b'a\x00c', b'a\xffc'], [b'ac', b'abbc']),
    (rb'a\.c\*\(\)\[\]\{\}\|\^\$\?\+\\', [b'a.c*()[]{}|^$?+\\'], [b'abc*()[]{}|^$?+\\']),
    (rb'a\t\r\f\v\a\0\x41\x7e', [b'a\t\r\f\v\a\x00A~'], [b'a\t\r\f\v\a\x00a~']),
    (rb'a\d\D\w\W\s\S', [b'a1x_- !'], [b'ax1_- !', b'a1x_-  ']),
    (rb'x[abc]y[^abc]z', [b'xbydz'], [b'xdydz', b'xbybz']),
    (rb'x[a-c0-2\-\]]y', [b'xby', b'x1y', b'x-y', b'x]y'], [b'xdy', b'x3y']),
    (rb'x[]a]y[^]a]z', [b'x]ybz', b'xaybz'], [b'xby', b'x]y]z']),
    (rb'x[\d\s\x41]y[\W]', [b'x5y!', b'x y-', b'xAy '], [b'xay!', b'x5ya']),
    (rb'x[a-]y[-a]z', [b'x-yaz', b'xay-z'], [b'xbyaz']),
    (rb'x(ab|cd)y', [b'xaby', b'xcdy'], [b'xy', b'xabcdy']),
    (rb'x(?:ab|cd|)y', [b'xaby', b'xy'], [b'xay']),
    (rb'x(a(b|c)d)*y', [b'xy', b'xabdacdy'], [b'xabd', b'xaby']),
    (rb'xa*y', [b'xy', b'xaaay'], [b'xby']),
    (rb'xa+y', [b'xay', b'xaay'], [b'xy']),
    (rb'xa?y', [b'xy', b'xay'], [b'xaay']),
    (rb'xa{3}y', [b'xaaay'], [b'xaay', b'xaaaay']),
    (rb'xa{2,}y', [b'xaay', b'xaaaaay'], [b'xay']),
    (rb'xa{1,2}y', [b'xay', b'xaay'], [b'xy', b'xaaay']),
    (rb'xa{,2}y', [b'xy', b'xaay'], [b'xaaay']),
    (rb'x(ab){2}y{0}z', [b'xababz'], [b'xabz', b'xababyz']),
    (rb'^ab', [b'ab', b'abc'], [b'xab']),
    (rb'ab$', [b'ab', b'xab'], [b'abx']),
    (rb'^ab$', [b'ab'], [b'abab', b'xab', b'abx']),
    (rb'^(a|b)c$', [b'ac', b'bc'], [b'abc', b'c']),
    (rb'^a.*b$', [b'ab', b'axxb', b'abab'], [b'aba']),
    (b'k\xc3\xa9z}]', [b'k\xc3\xa9z}]'], [b'k\xc3z}]']),
    (rb'a\ b\-c\/d\~', [b'a b-c/d~'], [b'ab-c/d~']),
]
ICASE = [
    (rb'HeLLo', [b'hello', b'HELLO'], [b'hell0']),
    (rb'x[^a]y', [b'xby', b'x@y'], [b'xay', b'xAy']),
    (rb'x[a-c]y', [b'xBy', b'xby'], [b'xdy', b'xDy']),
    (rb'x[Z-a]y', [b'xzy', b'xAy', b'x^y'], [b'xby', b'xYy']),
    (b'k\xc1z', [b'K\xc1Z'], [b'k\xe1z']),
    (rb'^x\wy$', [b'xAy', b'XaY'], [b'x-y']),
]
REFUSED = [
    (b'', 'empty pattern'), (b'a*?', 'lazy'), (b'a+?', 'lazy'), (b'a??', 'lazy'), (b'a{2}?', 'lazy'), (b'a*+', 'possessive'),
    (b'a{2}+', 'possessive'), (rb'(a)\1', 'back-reference'), (b'(?=a)b', 'look-around'), (b'(?!a)b', 'look-around'),
    (b'(?<=a)b', 'look-around'), (b'(?<!a)b', 'look-around'), (rb'a\b', r'\\b'), (rb'\Ba', r'\\b'), (rb'\Aa', r'\\b'), (rb'a\Z', r'\\b'),
    (b'(?i)a', 'inline flags'), (b'(?P<n>a)', 'named group'), (b'(?#c)a', 'inline flags'), (b'a^b', r'\^ anywhere'), (b'(^a)', r'\^ anywhere'),
    (b'a$b', r'\$ anywhere'), (b'(a$)', r'\$ anywhere'), (b'^a|b', 'bare alternation'), (b'a|b$', 'bare alternation'), (b'a{', 'malformed'),
    (b'a{1', 'malformed'), (b'a{,}', 'malformed'), (b'a{x}', 'malformed'), (b'a{}', 'malformed'), (b'a{2,1}', 'minimum is above'),
    (b'[a', 'without its ]'), (b'a[', 'without its ]'), (b'a[]', 'without its ]'), (b'x[z-a]', 'backwards'), (rb'x[a-\d]', 'end of a range'),
    (rb'x[\d-a]', 'end of a range'), (b'x[\xc3\xa9]', '>= 0x80'), (b'x[^\xff]', '>= 0x80'), (b'(a', 'without its \\)'), (b'a)', 'without its group'),
    (b'*a', 'nothing to repeat'), (b'a(*b)', 'nothing to repeat'), (b'a|*b', 'nothing to repeat'), (b'a**', 'repeat of a repeat'),
    (b'a{2}{3}', 'repeat of a repeat'), (rb'a\x4', 'two hex digits'), (rb'a\xg0', 'two hex digits'), (rb'a\01', 'octal'), (rb'a\e', 'unknown escape'),
    (rb'a\8', 'back-reference'), (b'a\\', 'ends in a backslash'), (rb'\d+', 'required literal'), (b'a|b', 'required literal'), (b'(ab)?', 'required literal'),
    (b'.*', 'required literal'), (b'[a]b*', 'required literal'), (b'^$', 'required literal'), (b'(a|b)c*', 'required literal'),
    (b'(' * 201 + b'a' + b')' * 201, 'nested more than 200 deep'), (b'(?:' * 200000 + b'a' + b')' * 200000, 'nested more than 200 deep'),
]
LITERALS = [
    (rb'(GET|POST) /api/v[0-9]+/users/\d+ 50[0-4]', [b' /api/v', b'/users/', b' 50']),
    (rb'user=\w+@example\.(com|org)', [b'@example.', b'user=']),
    (rb'^\d{4}-\d\d-\d\d .* timeout after \d+ ms$', [b' timeout after ', b' ms', b'-']),
    (rb'abc', [b'abc']), (rb'a(bc)d', [b'abcd']), (rb'a(?:bc){2}d', [b'abcbcd']), (rb'x(ab)+y', [b'xab', b'aby']), (rb'ab?c', [b'a', b'c']),
    (rb'(ab|cd)ef', [b'ef']), (rb'ab[c]de', [b'ab', b'de']), (rb'ab.de+f', [b'ab', b'de', b'ef']), (rb'a{2,}b', [b'ab']), (rb'(a.b){2}', [b'a', b'b']),
    (rb'one.two.three.four.five.six.seven.eight.nine.ten', [b'three', b'seven', b'eight', b'four', b'five', b'nine', b'one', b'two']),
    (rb'ab\x41\.c\n', [b'abA.c\n']), (rb'x(a*)yz', [b'yz', b'x']),
    # a literal may be far longer than its pattern: an exact {n} of up to 256 bytes is written out, and such runs join
    (rb'a{200}', [b'a' * 200]), (rb'(ab){128}', [b'ab' * 128]), (rb'a{200}b{200}c', [b'a' * 200 + b'b' * 200 + b'c']),
    (rb'x{256}\dy{256}', [b'x' * 256, b'y' * 256]), (rb'a{257}', [b'a']), (rb'(ab){129}c', [b'abc']),
]


def test_parser_table():
    for pat, yes, no in PARSER:
        for fold in (False, True):
            for s in yes + no:
                assert regex_match(pat, s, fold) == (re.search(pat, s, re.I if fold else 0) is not None), (pat, s, fold)
        assert all(regex_match(pat, s) for s in yes) and not any(regex_match(pat, s) for s in no), pat
    for pat, yes, no in ICASE:
        assert all(regex_match(pat, s, True) for s in yes) and not any(regex_match(pat, s, True) for s in no), pat
        for s in yes + no:
            assert regex_match(pat, s, True) == (re.search(pat, s, re.I) is not None), (pat, s)
    assert regex_match('kéz', 'xkéz'.encode()) and regex_literals('ké') == ['ké'.encode()]
    for text in (b'a.b*[c]\\d{2}(x|y)^$+?\n\x00\xff', bytes(b for b in range(256))):
        assert regex_literals(regex_escape(text)) == [text]
        entry = text.replace(b'\n', b'')                # (an entry holds no 0x0A)
        assert regex_match(regex_escape(entry), b'<' + entry + b'>') and not regex_match(regex_escape(entry), b'<' + entry[1:] + b'>')
    with pytest.raises(TypeError):
        regex_match(b'a', b'a', icase=1)
    with pytest.raises(TypeError):
        regex_literals(7)


@pytest.mark.parametrize('pat,what', REFUSED, ids=[repr(p[:40]) + str(len(p)) for p, _ in REFUSED])
def test_refusals_name_the_position(pat, what):
    for fn in (regex_literals, regex_info):
        with pytest.raises(ValueError, match=what) as e:
            fn(pat)
        assert 'at position' in str(e.value)
    with pytest.raises(ValueError, match=what):
        regex_match(pat, b'x', icase=True)


def test_host_matcher_against_re_on_the_seeded_pairs():
    pairs = [p for seed in SEEDS for p in make_regex_case(seed).pairs]
    assert len(pairs) >= 2000 and any(f for _, _, f in pairs) and any(not f for _, _, f in pairs)
    assert any(0 in s for _, s, _ in pairs) and any(max(s, default=0) >= 0x80 for _, s, _ in pairs)
    compiled, yes = {}, 0
    for pat, s, fold in pairs:
        key = (pat, fold)
        if key not in compiled:
            compiled[key] = (P._Regex(pat, fold), re.compile(pat, re.I if fold else 0))
        rx, ref = compiled[key]
        got = _ffi.lib.pss_regex_match(rx.handle, s, len(s))
        assert got == int(ref.search(s) is not None), (pat, s, fold, got)
        yes += got
    assert len(pairs) // 5 < yes < len(pairs) * 4 // 5


def test_literals():
    for pat, want in LITERALS:
        assert regex_literals(pat) == want, pat
    assert regex_literals(b'HeLLo \\d WORLD', True) == [b'hello ', b' world'] and regex_literals(b'x[a]Y', True) == [b'x', b'y']
    # sound: whatever re matches holds every literal
    rng = np.random.default_rng(5)
    for pat, _ in LITERALS[:13]:
        lits, rx = regex_literals(pat), re.compile(pat)
        for _ in range(200):
            s = bytes(rng.choice(np.frombuffer(b'abcdefxy .-0123456789', np.uint8), int(rng.integers(0, 24))))
            if rx.search(s):
                assert all(lit in s for lit in lits), (pat, s)


def test_state_cap():
    family = lambda n: b'x(a|b)*a(a|b){%d}' % n
    n = 1
    while True:
        try:
            info = regex_info(family(n))
        except ValueError as e:
            assert 'pattern too complex' in str(e) and '4096' in str(e)
            break
        assert info['states'] <= _ffi.REGEX_MAX_STATES and info['table_bytes'] == 2 * info['states'] * info['classes']
        n += 1
        assert n < 20
    assert n >= 8
    last = family(n - 1)
    assert regex_info(last)['states'] > _ffi.REGEX_MAX_STATES // 4
    rng = np.random.default_rng(6)
    rx = re.compile(last)
    for _ in range(300):
        s = b'x' + bytes(rng.choice(np.frombuffer(b'ab', np.uint8), int(rng.integers(0, 3 * n))))
        assert regex_match(last, s) == (rx.search(s) is not None), s


def test_position_cap():
    assert regex_info(b'a{2048}')['states'] == 2048 + 2 and regex_info(b'(ab){1024}')['states'] > 2048
    assert regex_match(b'^a{2048}$', b'a' * 2048) and not regex_match(b'^a{2048}$', b'a' * 2047)
    for pat in (b'a{2049}', b'(ab){1024}c', b'x(a{50}){41}', b'a{1,2049}', b'a{1000000}', b'((a{0}){100000}){100000}b'):
        with pytest.raises(ValueError, match='too complex'):
            regex_info(pat)


def _batch(patterns):
    blob = b''.join(patterns)
    offs = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in patterns])
    return blob, offs


def test_c_layer_refuses_without_a_reader():
    L = _ffi.lib
    out = ctypes.c_void_p()
    counts = np.full(3, 7, dtype=np.uint64)
    blob, offs = _batch([b'ab', b'a*?'])
    calls = [(L.pss_reader_search_regex_batch, lambda: ctypes.byref(out)), (L.pss_reader_search_regex_ids_batch, lambda: ctypes.byref(out)),
             (L.pss_reader_count_regex_batch, lambda: counts.ctypes.data)]
    for fn, o in calls:
        assert fn(None, blob, offs.ctypes.data, 2, 0, o()) == _ffi.PSS_EINVAL and 'pattern 1: a lazy quantifier' in _ffi.last_error()
        assert fn(None, blob, offs.ctypes.data, 1, 0, o()) == _ffi.PSS_EINVAL and 'no reader' in _ffi.last_error()      # a good batch: the reader, last
        assert fn(None, blob, offs.ctypes.data, 1, 4, o()) == _ffi.PSS_EINVAL and 'flags' in _ffi.last_error()
        assert fn(None, blob, offs.ctypes.data, 1, 0, None) == _ffi.PSS_EINVAL and 'bad arguments' in _ffi.last_error()
        assert fn(None, None, offs.ctypes.data, 1, 0, o()) == _ffi.PSS_EINVAL and 'bad arguments' in _ffi.last_error()
        assert fn(None, blob, None, 1, 0, o()) == _ffi.PSS_EINVAL and 'bad arguments' in _ffi.last_error()
        bad = np.array([1, 2], dtype=np.uint64)
        assert fn(None, blob, bad.ctypes.data, 1, 0, o()) == _ffi.PSS_EINVAL and 'start at 1' in _ffi.last_error()
        bad = np.array([0, 2, 1], dtype=np.uint64)
        assert fn(None, blob, bad.ctypes.data, 2, 0, o()) == _ffi.PSS_EINVAL and 'decrease at pattern 1' in _ffi.last_error()
    wide = b'x(a|b)*a(a|b){10}' + bytes(range(0x30, 0x5b)) + bytes(range(0x63, 0x7b))     # ~2100 states x ~70 classes x 2 bytes
    per = regex_info(wide)['table_bytes']
    many = (64 << 20) // per + 1
    big, boffs = _batch([wide] * many)
    assert L.pss_reader_count_regex_batch(None, big, boffs.ctypes.data, many, 0, counts.ctypes.data) == _ffi.PSS_EINVAL
    assert '64 MiB at pattern %d' % (many - 1) in _ffi.last_error()
    assert not out.value and counts.tolist() == [7] * 3
    rx = ctypes.c_void_p()
    assert L.pss_regex_compile(b'ab', 2, 0, None) == _ffi.PSS_EINVAL and L.pss_regex_compile(None, 2, 0, ctypes.byref(rx)) == _ffi.PSS_EINVAL
    assert L.pss_regex_compile(b'ab', 2, 2, ctypes.byref(rx)) == _ffi.PSS_EINVAL and not rx.value
    assert L.pss_regex_compile(b'ab', 2, 0, ctypes.byref(rx)) == _ffi.PSS_OK and rx.value
    info, n, offs9 = _ffi.RegexDfa(), ctypes.c_uint32(), (ctypes.c_uint64 * 9)()
    buf = ctypes.create_string_buffer(8)
    assert L.pss_regex_info(None, ctypes.byref(info)) == _ffi.PSS_EINVAL and L.pss_regex_info(rx, None) == _ffi.PSS_EINVAL
    assert L.pss_regex_literals(rx, buf, 1, offs9, ctypes.byref(n)) == _ffi.PSS_EINVAL and L.pss_regex_literals(None, buf, 8, offs9, ctypes.byref(n)) == _ffi.PSS_EINVAL
    assert L.pss_regex_literals(rx, buf, 8, offs9, ctypes.byref(n)) == _ffi.PSS_OK and n.value == 1 and buf.raw[:2] == b'ab' and list(offs9[:2]) == [0, 2]
    offs9[1], n.value = 99, 9                             # the size query: no buffer, the offsets and the count alone
    assert L.pss_regex_literals(rx, None, 0, offs9, ctypes.byref(n)) == _ffi.PSS_OK and n.value == 1 and list(offs9[:2]) == [0, 2]
    assert L.pss_regex_literals(rx, None, 8, offs9, ctypes.byref(n)) == _ffi.PSS_EINVAL
    long_rx = ctypes.c_void_p()
    long_pat = rb'a{200}\db{3}'
    assert L.pss_regex_compile(long_pat, len(long_pat), 0, ctypes.byref(long_rx)) == _ffi.PSS_OK
    assert L.pss_regex_literals(long_rx, None, 0, offs9, ctypes.byref(n)) == _ffi.PSS_OK and n.value == 2 and list(offs9[:3]) == [0, 200, 203]
    big = ctypes.create_string_buffer(203)
    assert L.pss_regex_literals(long_rx, big, 202, offs9, ctypes.byref(n)) == _ffi.PSS_EINVAL and '203 bytes' in _ffi.last_error()
    assert L.pss_regex_literals(long_rx, big, 203, offs9, ctypes.byref(n)) == _ffi.PSS_OK and big.raw == b'a' * 200 + b'bbb'
    L.pss_regex_free(long_rx)
    assert L.pss_regex_match(None, b'ab', 2) == _ffi.PSS_EINVAL and L.pss_regex_match(rx, None, 2) == _ffi.PSS_EINVAL
    assert L.pss_regex_match(rx, b'xab', 3) == 1 and L.pss_regex_match(rx, b'xa', 2) == 0 and L.pss_regex_match(rx, None, 0) == 0
    L.pss_regex_free(rx)
    L.pss_regex_free(None)


def test_info_keeps_the_numbering_contract():
    a, b = regex_info(b'ab+c'), regex_info(b'^ab+c$')
    assert a['anchors'] == 0 and a['sink'] == a['first_accept'] == a['states'] - 1 and a['start'] == 1
    assert b['anchors'] == 3 and b['sink'] == 0 and 1 <= b['first_accept'] < b['states'] and regex_info(b'^ab')['anchors'] == 1
    assert regex_info(b'AB', True)['classes'] == 4 and regex_info(b'AB')['classes'] == 4      # A, B, 0x0A, the rest


def test_the_names_are_in_the_stubs_and_the_header():
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in ('search_regex', 'count_regex', 'search_regex_ids_batch', 'search_regex_batch_packed', 'count_regex_bytes'):
        par = inspect.signature(getattr(P.Reader, name)).parameters['icase']
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False, name
        assert '*, icase: bool = False' in next(ln for ln in stub.splitlines() if f'def {name}(' in ln), name
    for name in ('regex_literals', 'regex_info', 'regex_match', 'regex_escape'):
        assert name in P.__all__ and f'def {name}(' in stub
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    for name in ('pss_regex_compile', 'pss_regex_info', 'pss_regex_literals', 'pss_regex_match', 'pss_reader_search_regex_batch',
                 'pss_reader_search_regex_ids_batch', 'pss_reader_count_regex_batch'):
        assert f'int {name}(' in hdr and hasattr(_ffi.lib, name)
    assert 'void pss_regex_free(' in hdr and '#define PSS_REGEX_ICASE 1u' in hdr and '#define PSS_REGEX_MAX_STATES 4096u' in hdr
    assert not hasattr(__import__('pysubstringsearch_amd.dist', fromlist=['x']).ShardedReader, 'search_regex_ids_batch')


def test_compiler_under_sanitizers(tmp_path):
    """csrc/regex_compile.h and the RegexBlock of csrc/search_layout.h alone, built with g++ under AddressSanitizer + UBSan
    (tests/native/regex_compile.cpp): the seeded patterns with the answers of Python's re, the parser table and every refusal."""
    lines = []
    hx = lambda b: b.hex() if b else '-'
    for seed in SEEDS:
        by_pattern = {}
        for pat, s, fold in make_regex_case(seed).pairs:
            by_pattern.setdefault((pat, fold), []).append(s)
        for (pat, fold), strings in by_pattern.items():
            rx = re.compile(pat, re.I if fold else 0)
            lines.append(' '.join([str(int(fold)), 'accept', hx(pat)] + ['%s %d' % (hx(s), rx.search(s) is not None) for s in strings]))
    for pat, yes, no in PARSER:
        lines.append(' '.join(['0', 'accept', hx(pat)] + ['%s 1' % hx(s) for s in yes] + ['%s 0' % hx(s) for s in no]))
    for pat, _ in REFUSED:
        lines += ['%d refuse %s' % (f, hx(pat)) for f in (0, 1)]
    lines += ['0 refuse ' + hx(b'x(a|b)*a(a|b){13}'), '0 refuse ' + hx(b'a{2049}'), '0 accept ' + hx(b'x(a|b)*a(a|b){11}') + ' ' + hx(b'xab' + b'a' * 11) + ' 1']
    cases = tmp_path / 'cases.txt'
    cases.write_text('\n'.join(lines) + '\n')
    csrc = os.path.join(ROOT, 'pysubstringsearch_amd', 'csrc')
    exe = str(tmp_path / 'regex_compile')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I' + csrc,
                        os.path.join(ROOT, 'tests', 'native', 'regex_compile.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'regex_compile: ok' in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
