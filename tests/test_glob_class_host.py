"""Host side of the wildcard search with byte classes (`?`, `[set]`, `[!set]` behind classes=True): the pattern language,
the core rule, the reference and the case generator.  No GPU: tests/test_glob_class_gpu.py runs the engine."""
import ctypes
import fnmatch
import inspect
import os
import pathlib
import random

import numpy as np
import pytest

from tests.glob_class_fuzz_cases import PER_BATCH, SEEDS, make_case
from tests.glob_class_ref import GlobClassRef, negated_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = bytes(b for b in range(256) if b != 0x0A)
METHODS = ('search_glob_batch_packed', 'search_glob_ids_batch', 'count_glob_bytes', 'search_glob', 'count_glob')


def lits(b):
    return [bytes([x]) for x in b]


def without(*drop):
    return bytes(b for b in range(256) if b not in drop and b != 0x0A)


PARSED = [
    (b'a?c', ([[b'a', ANY, b'c']], 3)),
    (b'a**?b', ([[b'a'], [ANY, b'b']], 3)),
    (b'*a\\?*', ([[b'a', b'?']], 0)),
    (b'[]a]x', ([[b']a', b'x']], 3)),
    (b'x[!]]', ([[b'x', without(0x5D)]], 3)),
    (b'x[^a]', ([[b'x', b'^a']], 3)),
    (b'x[a-]*', ([[b'x', b'-a']], 1)),
    (b'*x[-a]', ([[b'x', b'-a']], 2)),
    (b'x[!-a]', ([[b'x', without(0x2D, 0x61)]], 3)),
    (b'x[\\]]', ([[b'x', b']']], 3)),
    (b'x[*]', ([[b'x', b'*']], 3)),
    (b'x[?][[]', ([[b'x', b'?', b'[']], 3)),
    (b'[a-c]x[0-2]', ([[b'abc', b'x', b'012']], 3)),
    (b'x[\x80-\x82\xff]', ([[b'x', b'\x80\x81\x82\xff']], 3)),
    (b'x[\x00a]', ([[b'x', b'\x00a']], 3)),
    (b'x[\x09-\x0b]', ([[b'x', b'\x09\x0b']], 3)),                 # the newline leaves every set
    (b'x[!\x00-\x7f]', ([[b'x', bytes(range(0x80, 0x100))]], 3)),
    (b'x[\\a-\\c]', ([[b'x', b'abc']], 3)),
    (b'x]y', ([[b'x', b']', b'y']], 3)),
    (b'a\nb?', ([[b'a', b'\n', b'b', ANY]], 3)),                   # a literal newline stays (it voids the pattern in a search)
    (b'*??*ab*', ([[ANY, ANY], [b'a', b'b']], 0)),
]


@pytest.mark.parametrize('pattern,want', PARSED)
def test_parser(pattern, want):
    from pysubstringsearch_amd import glob_parse
    assert glob_parse(pattern, classes=True) == want
    assert glob_parse(pattern, True) == want and glob_parse(bytearray(pattern), classes=True) == want


@pytest.mark.parametrize('pattern,what', [
    (b'ab[cd', 'not closed'), (b'ab[', 'not closed'), (b'ab[]', 'not closed'), (b'ab[!]', 'not closed'), (b'ab[a-', 'not closed'),
    (b'ab[\n]', 'empty'), (b'ab[!\x00-\xff]', 'empty'),
    (b'ab[z-a]', 'descends'), (b'ab[b-\\a]', 'descends'),
    (b'ab\\', 'lone backslash'), (b'ab[c\\', 'lone backslash'),
    (b'???', 'nothing in the suffix array'), (b'*[0-9]*', 'nothing in the suffix array'), (b'?*?', 'nothing in the suffix array'),
    (b'', 'no literal byte'), (b'*', 'no literal byte'), (b'[ab][cd]', 'no literal byte'),
])
def test_parser_errors(pattern, what):
    from pysubstringsearch_amd import glob_cores, glob_parse
    with pytest.raises(ValueError, match=what) as err:
        glob_parse(pattern, classes=True)
    assert repr(pattern) in str(err.value)
    with pytest.raises(ValueError, match=what):
        glob_cores(pattern)
    with pytest.raises(TypeError):
        glob_parse(pattern.decode('latin-1'), classes=True)


def test_escape_round_trip_on_all_bytes():
    from pysubstringsearch_amd import glob_escape, glob_parse
    x = bytes(range(256))
    assert glob_parse(glob_escape(x, classes=True), classes=True) == ([lits(x)], 3)
    for b in range(256):
        assert glob_parse(glob_escape(bytes([b]), classes=True), classes=True) == ([[bytes([b])]], 3)
    assert glob_escape(b'a?[b]*\\', classes=True) == b'a\\?\\[b\\]\\*\\\\'
    with pytest.raises(TypeError):
        glob_escape('a', classes=True)


def test_without_the_keyword_nothing_changes():
    from pysubstringsearch_amd import glob_escape, glob_parse
    for p, want in ((b'a?[b]', ([b'a?[b]'], 3)), (b'*[!x]?*]', ([b'[!x]?', b']'], 2)), (b'[*]', ([b'[', b']'], 3)), (b'??', ([b'??'], 3)),
                    (b'[z-a', ([b'[z-a'], 3))):
        assert glob_parse(p) == want and glob_parse(p, classes=False) == want and glob_parse(p, False) == want
    assert glob_escape(b'a?[b]*\\') == glob_escape(b'a?[b]*\\', classes=False) == b'a?[b]\\*\\\\'
    assert list(inspect.signature(glob_parse).parameters)[:2] == ['pattern', 'classes']
    assert inspect.signature(glob_parse).parameters['classes'].default is False
    assert inspect.signature(glob_escape).parameters['classes'].default is False


def test_fold_closes_what_is_written_before_it_negates():
    from pysubstringsearch_amd import glob_parse
    segs, a = glob_parse(b'x[a-c][!a]?[Q1]', classes=True, fold=True)
    assert a == 3 and segs == [[b'x', b'ABCabc', without(0x41, 0x61), ANY, b'1Qq']]
    assert glob_parse(b'x[a-c]', classes=True)[0] == [[b'x', b'abc']]
    assert glob_parse(b'x[a]?[a-a]', classes=True, fold=True) == glob_parse(b'x[a]?[a-a]', classes=True) == ([[b'x', b'a', ANY, b'a']], 3)
    ref = GlobClassRef([b'xBq\nxbA\n'])
    assert ref.parsed(b'x[a-c][!a]', fold=True)[0] == [[b'Xx', b'ABCabc', without(0x41, 0x61)]]
    assert negated_positions(b'a[!x]*[]!]\\[[!]]') == [[False, True], [False, False, True]]


def test_cores():
    from pysubstringsearch_amd import glob_cores
    assert glob_cores(b'ab?cd') == [(0, b'ab')]                           # a tie: the leftmost
    assert glob_cores(b'a?bcd?ef') == [(2, b'bcd')]
    assert glob_cores(b'?ab?cde?fgh') == [(4, b'cde')]
    assert glob_cores(b'*??*ab*[0-9][!x]*[*]') == [None, (0, b'ab'), None, (0, b'*')]
    assert glob_cores(b'[0-9]x') == [(1, b'x')]
    assert glob_cores(b'\\?\\[?') == [(0, b'?[')]
    assert glob_cores(b'a' * 70 + b'?' + b'b' * 70) == [(0, b'a' * 70)]


def test_c_layer_derives_the_same_cores():
    from pysubstringsearch_amd import _ffi, _glob_class_args, glob_cores
    rnd = random.Random(5)
    patterns = [b'ab?cd', b'a?bcd?ef', b'*??*ab*[0-9][!x]*[*]', b'[0-9]x', b'x' + b'?' * 9 + b'yz?' + b'q' * 65]
    for _ in range(200):
        body = b''.join(rnd.choice((b'a', b'b', b'?', b'[xy]', b'*', b'\\*', b'[!a]')) for _ in range(rnd.randrange(1, 14)))
        patterns.append(b'z' + body)
    args, keep = _glob_class_args(patterns, False)
    nsegs = args[3]
    off, ln = np.zeros(nsegs, dtype=np.uint32), np.zeros(nsegs, dtype=np.uint32)
    _ffi.check(_ffi.lib.pss_seqc_cores(args[1], args[2], nsegs, off.ctypes.data, ln.ctypes.data))
    want = [c for p in patterns for c in glob_cores(p)]
    assert len(want) == nsegs
    soff = keep[2].tolist()
    for t, core in enumerate(want):
        if core is None:
            assert ln[t] == 0
        else:
            assert (int(off[t]), keep[0][soff[t] + off[t]:soff[t] + off[t] + ln[t]]) == core


def test_batches_are_packed_for_the_library():
    from pysubstringsearch_amd import SEQ_MAX_SETS, _ffi, _glob_class_args
    args, keep = _glob_class_args([b'a?c*[0-9]x', b'*??*b[0-9]', b'q\\?'], False)
    lit, plane, soffs, sets, goffs, anch = keep
    assert lit == b'a\0c\0x\0\0b\0q?' and plane == b'\0\1\0\2\0\1\1\0\2\0\0'
    assert soffs.tolist() == [0, 3, 5, 7, 9, 11] and goffs.tolist() == [0, 2, 4, 5] and anch.tolist() == [3, 2, 3]
    assert args[3] == 5 and args[5] == 2 and args[7] == 3 and args[9] == 0
    member = lambda k, b: bool(sets[k - 1][b >> 3] >> (b & 7) & 1)
    assert [b for b in range(256) if member(1, b)] == list(ANY) and [b for b in range(256) if member(2, b)] == list(b'0123456789')
    assert _glob_class_args([b'a[b-c]'], True)[0][9] == _ffi.SEQ_FOLD == 1
    args, keep = _glob_class_args([], False)
    assert args[3] == 0 and args[7] == 0 and keep[2].tolist() == [0] and keep[4].tolist() == [0]
    many = [b'x' + b''.join(b'[' + bytes([65 + i // 26, 97 + i % 26]) + b']' for i in range(j, j + 8)) for j in range(0, 256, 8)]
    _glob_class_args(many[:31] + [b'x[ab][cd][ef][gh][ij][kl][mn]'], False)             # 255 sets
    with pytest.raises(ValueError, match=str(SEQ_MAX_SETS)):
        _glob_class_args(many, False)


def test_the_keyword_is_on_the_five_methods_and_in_the_stubs():
    import pysubstringsearch_amd as P
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in METHODS:
        method = getattr(P.Reader, name)
        assert 'classes' not in inspect.signature(method).parameters
        par = inspect.signature(method, follow_wrapped=False).parameters['classes']
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False, name
        assert '``classes=True``' in method.__doc__ and method.__name__ == name
        line = next(ln for ln in stub.splitlines() if f'def {name}(' in ln)
        assert '*, icase: bool = False, classes: bool = False' in line, name
    for name in ('search_all_batch_packed', 'search_all_ids_batch', 'count_all_bytes', 'search_all', 'count_all'):
        assert 'classes' not in inspect.signature(getattr(P.Reader, name), follow_wrapped=False).parameters
    assert not hasattr(__import__('pysubstringsearch_amd.dist', fromlist=['x']).ShardedReader, 'search_glob_ids_batch')
    assert 'glob_cores' in P.__all__ and 'def glob_cores(' in stub and 'classes' in next(ln for ln in stub.splitlines() if 'def glob_escape(' in ln)
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    for name in ('pss_reader_search_seqc_batch', 'pss_reader_search_seqc_ids_batch', 'pss_reader_count_seqc_batch', 'pss_seqc_cores'):
        assert f'int {name}(' in hdr and hasattr(P._ffi.lib, name)
    assert '#define PSS_SEQ_FOLD 1u' in hdr


def test_bad_arguments_are_refused_before_the_library_is_called():
    import pysubstringsearch_amd as P
    r = P.Reader._from_handle(ctypes.c_void_p())      # (closed: reaching the library would raise 'closed Reader' instead)
    for call in (r.search_glob_batch_packed, r.search_glob_ids_batch, r.count_glob_bytes):
        for bad, what in (([b'a', b'??'], 'nothing in the suffix array'), ([b'a[b'], 'not closed'), ([b'a[]'], 'not closed'), ([b'a\\'], 'lone backslash')):
            with pytest.raises(ValueError, match=what):
                call(bad, classes=True)
            with pytest.raises(ValueError, match=what):
                call(bad, classes=True, icase=True)
        for bad in (b'a?b', 'a?b', ['a?b']):
            with pytest.raises(TypeError):
                call(bad, classes=True)
        with pytest.raises(TypeError, match='classes'):
            call([b'a'], classes=1)
        with pytest.raises(ValueError, match='closed Reader'):
            call([b'a?'], classes=True)
        with pytest.raises(ValueError, match='closed Reader'):
            call([b'a[b'], classes=False)             # without the keyword `[` is a byte
    with pytest.raises(ValueError, match='nothing in the suffix array'):
        r.search_glob('??', classes=True)
    with pytest.raises(ValueError, match='nothing in the suffix array'):
        r.count_glob('*[0-9]*', classes=True, icase=True)
    with pytest.raises(TypeError):
        r.search_glob(b'a?', classes=True)


def c_args(segs, planes, sets, goff, anch, flags=0):
    """The arguments of a pss_reader_search_seqc_* call between the reader and the output, and what they point into."""
    lit, plane = b''.join(segs), b''.join(planes)
    soffs = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
    table = np.zeros((max(len(sets), 1), 32), dtype=np.uint8)
    for k, members in enumerate(sets):
        for b in members:
            table[k][b >> 3] |= 1 << (b & 7)
    g, a = np.array(goff, dtype=np.uint64), np.array(anch if anch else [0], dtype=np.uint8)
    keep = (lit, plane, soffs, table, g, a)
    return (lit, plane, soffs.ctypes.data, len(segs), table.ctypes.data, len(sets), g.ctypes.data, len(goff) - 1, a.ctypes.data, flags), keep


BAD_C_BATCHES = [
    ('no segment', c_args([b'a', b'b'], [b'\0', b'\0'], [], [0, 0, 2], [0, 0])),
    ('is empty', c_args([b'a', b''], [b'\0', b''], [], [0, 2], [0])),
    ('anchors[0] = 4', c_args([b'a'], [b'\0'], [], [0, 1], [4])),
    ('group offsets', c_args([b'a', b'b'], [b'\0', b'\0'], [], [1, 2], [0])),
    ('group offsets', c_args([b'a', b'b'], [b'\0', b'\0'], [], [0, 3, 2], [0, 0])),
    ('names set 2', c_args([b'a\0'], [b'\0\2'], [b'xy'], [0, 1], [0])),
    ('names set 1', c_args([b'a\0'], [b'\0\1'], [], [0, 1], [0])),
    ('under a class index', c_args([b'ab'], [b'\0\1'], [b'xy'], [0, 1], [0])),
    ('holds 0x0A', c_args([b'a\0'], [b'\0\1'], [b'x\n'], [0, 1], [0])),
    ('set 2 is empty', c_args([b'a\0'], [b'\0\1'], [b'x', b''], [0, 1], [0])),
    ('no segment with a literal byte', c_args([b'a', b'\0\0'], [b'\0', b'\1\1'], [b'xy'], [0, 1, 2], [0, 0])),
    ('closed under the fold', c_args([b'a\0'], [b'\0\1'], [b'xY'], [0, 1], [0], flags=1)),
    ('closed under the fold', c_args([b'a\0'], [b'\0\1'], [bytes(b for b in range(256) if b not in (0x0A, 0x61))], [0, 1], [0], flags=1)),
    ('flags = 0x2', c_args([b'a'], [b'\0'], [], [0, 1], [0], flags=2)),
]


@pytest.mark.parametrize('what,packed', BAD_C_BATCHES)
def test_bad_batches_are_refused_by_the_c_calls(what, packed):
    """PSS_EINVAL with a message, *out and counts untouched.  The batch is judged before the reader is, so no device is
    needed; tests/test_glob_class_gpu.py repeats the calls on a live reader."""
    from pysubstringsearch_amd import _ffi
    args, keep = packed
    for fn in (_ffi.lib.pss_reader_search_seqc_batch, _ffi.lib.pss_reader_search_seqc_ids_batch):
        out = ctypes.c_void_p()
        assert fn(None, *args, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert not out.value and what in _ffi.last_error(), _ffi.last_error()
    counts = np.full(4, 7, dtype=np.uint64)
    assert _ffi.lib.pss_reader_count_seqc_batch(None, *args, counts.ctypes.data) == _ffi.PSS_EINVAL
    assert counts.tolist() == [7] * 4 and what in _ffi.last_error()


def test_good_batches_and_null_arguments_without_a_reader():
    from pysubstringsearch_amd import _ffi
    out = ctypes.c_void_p()
    args, keep = c_args([b'a\0'], [b'\0\1'], [b'xY'], [0, 1], [3])            # not closed under the fold: fine without the flag
    assert _ffi.lib.pss_reader_search_seqc_batch(None, *args, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert 'no reader' in _ffi.last_error() and 'pss_reader_search_seqc_batch' in _ffi.last_error()
    assert _ffi.lib.pss_reader_search_seqc_ids_batch(None, *args, None) == _ffi.PSS_EINVAL and 'no reader' not in _ffi.last_error()
    assert _ffi.lib.pss_reader_count_seqc_batch(None, *args, None) == _ffi.PSS_EINVAL and 'no reader' not in _ffi.last_error()
    for hole in (0, 1, 2, 4, 6, 8):
        bad = list(args)
        bad[hole] = None
        assert _ffi.lib.pss_reader_search_seqc_batch(None, *bad, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert 'bad arguments' in _ffi.last_error() and not out.value


# ---- the reference, judged by fnmatch ----------------------------------------------------------------------------------

def _fnmatch_cases():
    rnd = random.Random(20)
    alphabet = b'abcxyz019-]^!.'
    entries = [bytes(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 9))) for _ in range(300)]
    full = [e for e in entries if len(e) >= 2]
    patterns = []
    while len(patterns) < 400:
        e = rnd.choice(full)
        a, b = sorted(rnd.sample(range(len(e) + 1), 2))
        out = [b'*'] if a and rnd.random() < 0.8 else []
        lit = False
        for x in e[a:b]:
            roll = rnd.random()
            if roll < 0.4 and x not in b'[]*?':
                out.append(bytes([x]))
                lit = True
            elif roll < 0.55:
                out.append(b'?')
            elif roll < 0.62:
                out.append(b'*')
            else:
                first = b']' if rnd.random() < 0.15 else b''
                mid = bytes(rnd.choice(b'abcxyz019^.') for _ in range(rnd.randrange(0, 3)))
                rng = rnd.choice((b'', b'a-c', b'0-9', b'x-z', b'.-9'))
                last = b'-' if rnd.random() < 0.15 else b''
                body = first + mid + rng + last or b'a'
                if rnd.random() < 0.5:
                    body += bytes([x]) if x not in b']-^!' else b''
                neg = b'!' if rnd.random() < 0.3 else b''
                if not neg and body[:1] == b'!':
                    body = body[1:] + b'!'
                out.append(b'[' + neg + (body or b'a') + b']')
        if b < len(e) and rnd.random() < 0.8:
            out.append(b'*')
        if lit:
            patterns.append(b''.join(out))
    return entries, patterns


def test_the_reference_agrees_with_fnmatch():
    """An oracle the parser did not write: fnmatch.fnmatchcase on bytes against the reference through glob_parse, for
    patterns without a backslash, a descending range, an unclosed bracket or a newline."""
    from pysubstringsearch_amd import glob_parse
    entries, patterns = _fnmatch_cases()
    assert len(patterns) == 400 and len(set(patterns)) > 300
    text = b''.join(e + b'\n' for e in entries)
    ref = GlobClassRef([text])
    some = none = 0
    for p in patterns:
        assert b'\\' not in p and b'\n' not in p
        want = [i for i, e in enumerate(entries) if fnmatch.fnmatchcase(e, p)]
        got = ref.search_class_ids(*glob_parse(p, classes=True)).tolist()
        assert got == want, p
        some += bool(want)
        none += len(want) < len(entries)
    assert some >= len(patterns) // 2 and none >= len(patterns) // 2, (some, none)


# ---- the case generator ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', list(SEEDS))
def test_the_fuzz_cases_mix_what_they_should(seed):
    from pysubstringsearch_amd import glob_cores, glob_parse
    case = make_case(seed)
    assert case == make_case(seed) and len(case.patterns) == PER_BATCH
    ref = GlobClassRef(case.chunks)
    kinds = {'?': 0, 'set': 0, 'negated': 0, 'coreless': 0}
    anchors = set()
    matched = folded = 0
    for p in case.patterns:
        segs, a = glob_parse(p, classes=True)
        anchors.add(a)
        neg = negated_positions(p)
        for seg, ns in zip(segs, neg):
            for pos, n in zip(seg, ns):
                kinds['?'] += pos == ANY
                kinds['negated'] += n
                kinds['set'] += not n and 1 < len(pos) < 255
        kinds['coreless'] += sum(c is None for c in glob_cores(p))
        matched += ref.search_glob_ids(p).size > 0
        folded += ref.search_glob_ids(p, fold=True).size > 0
    assert all(kinds.values()), kinds
    assert anchors == {0, 1, 2, 3}
    assert matched >= PER_BATCH // 2 and folded >= PER_BATCH // 2, (matched, folded)


def test_the_reference_states_the_driver():
    text = b'abab xq\nab xq\nzz\n'
    ref = GlobClassRef([text, b'ab\n'])
    assert ref.core_hits(0, b'ab', False) == 3 and ref.core_hits(0, b'xq', False) == 2
    assert ref.driver(0, b'ab?*x[p-r]') == (1, 2) and ref.driver(1, b'ab?*x[p-r]') == (None, 0)
    assert ref.driver(0, b'a[b]*?b') == (0, 3)                      # a tie (`ab` and `b` occur three times each): the lowest index
    assert ref.hits([b'ab?*x[p-r]', b'*??*zz']) == 2 + 0 + 1 + 0
    assert ref.hits([b'a\nb?']) == 0
    assert ref.search_glob_ids(b'ab?b*x[p-r]').tolist() == [0] and ref.search_glob_ids(b'AB?*X[p-r]', fold=True).tolist() == [0, 1]
    assert ref.search_glob_ids(b'*[!a-z]*q').tolist() == [0, 1]
    assert ref.search_glob_ids(b'*??*z').tolist() == [] and ref.search_glob_ids(b'?z').tolist() == [2]
