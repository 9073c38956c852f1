"""The case-insensitive all-terms and wildcard search without a device: the brute-force reference of
tests/icase_groups_ref.py against hand-written cases, the surface (C symbols, ctypes mirror, the ``icase`` keyword) and
the Python argument errors that are raised before the library is called."""
import ctypes
import inspect
import os
import pathlib

import numpy as np
import pytest

from tests.icase_groups_ref import IcaseGroupsRef, holds_all, matches_glob, matches_seq, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS_0X20 = ((b'@', b'`'), (b'[', b'{'), (b'\\', b'|'), (b'\xc1', b'\xe1'), (b'\x00', b' '), (b']', b'}'), (b'^', b'~'), (b'\xd0', b'\xf0'))
ALL_METHODS = ('search_all_ids_batch', 'search_all_batch_packed', 'count_all_bytes', 'search_all', 'count_all')
GLOB_METHODS = ('search_glob_ids_batch', 'search_glob_batch_packed', 'count_glob_bytes', 'search_glob', 'count_glob')
SYMBOLS = ('pss_reader_search_terms_icase_batch', 'pss_reader_search_terms_icase_ids_batch', 'pss_reader_count_terms_icase_batch',
           'pss_reader_search_seq_icase_batch', 'pss_reader_search_seq_icase_ids_batch', 'pss_reader_count_seq_icase_batch')


def test_the_pairs_are_the_ones_the_plain_icase_tests_use():
    from tests import icase_texts
    assert PAIRS_0X20 == icase_texts.PAIRS_0X20


# ---- the reference against hand-written cases -----------------------------------------------------------------------------

def test_all_terms_by_hand():
    g = ([b'Error', b'TIMEOUT'], [b'retry'])
    assert holds_all(b'ERROR: timeout', g) and holds_all(b'a TimeOut after an eRRoR', g)
    assert not holds_all(b'error: timeout, RETRY', g) and not holds_all(b'error: time out', g) and not holds_all(b'timeout', g)
    assert holds_all(b'xay', [b'A']) and not holds_all(b'xay', ([b'a'], [b'Y']))
    # a void include term empties the group, a void exclude term is ignored
    assert not holds_all(b'ab', [b'a', b'a\nb']) and holds_all(b'ab', ([b'A'], [b'a\nb']))
    # a bare sequence is a group without exclusions; a term may repeat
    assert holds_all(b'aB', [b'ab', b'AB', b'b'])
    # only ASCII letters fold
    assert holds_all('Été'.encode(), ['ÉTé'.encode()]) and not holds_all('Été'.encode(), ['été'.encode()])
    assert not holds_all('é'.encode(), ['É'.encode()]) and holds_all('É x'.encode(), ['É'.encode(), b'X'])


def test_glob_by_hand():
    assert not matches_glob(b'a', b'a*A') and matches_glob(b'aa', b'a*A') and matches_glob(b'AxA', b'a*a')
    assert matches_glob(b'abBA', b'ab*BA') and not matches_glob(b'aBa', b'ab*BA') and matches_glob(b'ABxxba', b'ab*BA')
    assert matches_glob(b'GET /x/Admin/y 500', b'get */ADMIN* 500') and not matches_glob(b'GET /x/Admin/y 5000', b'get */ADMIN* 500')
    assert not matches_glob(b'FORGET /admin 500', b'get */ADMIN* 500') and matches_glob(b'FORGET /admin 500', b'*get */ADMIN* 500')
    # one segment, both anchors: the entry equals it under fold
    assert matches_glob(b'HeLLo', b'hello') and not matches_glob(b'HeLLo!', b'hello') and not matches_glob(b' hello', b'HELLO')
    assert matches_glob(b'HeLLo!', b'hello*') and matches_glob(b' hello', b'*HELLO')
    # in order and without overlap
    assert not matches_glob(b'aba', b'*AB*BA*') and matches_glob(b'abba', b'*AB*BA*') and not matches_glob(b'ba ab', b'*AB*BA*')
    assert matches_seq(b'xAbY', [b'a', b'B'], 0) and not matches_seq(b'xAbY', [b'a', b'B'], 1) and matches_seq(b'AbY', [b'a', b'B'], 1)
    assert not matches_seq(b'ab', [b'a', b'b\n'], 0)
    assert not matches_glob('é'.encode(), 'É'.encode()) and matches_glob('xé'.encode(), 'Xé'.encode())
    # an escaped star is a byte like any other
    assert matches_glob(b'A*b', b'a\\*B') and not matches_glob(b'Axb', b'a\\*B')


@pytest.mark.parametrize('lo,hi', PAIRS_0X20)
def test_bytes_that_differ_by_0x20_and_are_no_letters(lo, hi):
    assert not holds_all(b'x' + lo + b'y', [b'X', hi]) and holds_all(b'x' + lo + b'y', [b'Y', lo])
    assert holds_all(b'x' + lo + b'y', ([b'X'], [hi])) and not holds_all(b'x' + lo + b'y', ([b'X'], [lo]))
    esc = lambda b: b'\\' + b if b in (b'\\', b'*') else b
    assert matches_glob(b'x' + lo + b'y', b'X' + esc(lo) + b'*Y') and not matches_glob(b'x' + lo + b'y', b'X' + esc(hi) + b'*Y')
    assert matches_glob(b'Q' + hi + hi, b'*q*' + esc(hi)) and not matches_glob(b'Q' + hi + hi, b'*q*' + esc(lo))


def test_ids_driver_hits_and_order_by_hand():
    #          0        1          2      3          4       (chunk 0)              0           1        (chunk 1, unterminated)
    texts = [b'zz AB\nab zz Zz\nzz\nAb aB zZ\nAB\n', b'ZZ ab\nzz Ab zz ab']
    ref = IcaseGroupsRef(texts)
    assert ref.search_all_ids([b'ab', b'ZZ']).tolist() == [0, 1, 3, 1 << 32, (1 << 32) | 1]
    assert ref.search_all_ids(([b'ab'], [b'Zz'])).tolist() == [4]
    assert ref.search_glob_ids(b'*zz*AB*').tolist() == [0, 1 << 32, (1 << 32) | 1]
    assert ref.search_glob_ids(b'ab*ZZ').tolist() == [1, 3]
    assert ref.search_glob_ids(b'*AB').tolist() == [0, 4, 1 << 32, (1 << 32) | 1]          # the last byte of the open entry takes part
    # seed hits: `ab` 5 / 3, `zz` 5 / 3 -> a tie goes to the lowest index; with `z` (6 / 6 ... more) the other term drives
    assert (seed_of(b'ab'), seed_of(b'Zz')) == ((0, b'AB'), (0, b'ZZ'))
    assert [ref.seed_hits(c, b'ab') for c in (0, 1)] == [5, 3] and [ref.seed_hits(c, b'zz') for c in (0, 1)] == [5, 3]
    assert ref.drivers('all', [b'zz', b'ab']) == [0, 0] and ref.drivers('all', [b'z', b'ab']) == [1, 1]
    assert ref.hits('all', [[b'zz', b'ab'], ([b'ab'], [b'zz']), [b'ab', b'a\nb'], [b'ab', b'nope']]) == 8 + 8 + 0 + 0
    assert ref.drivers('glob', b'*nope*ab*') == [None, None]
    # order: the suffixes at the driver's leftmost match -- 'AB\n..' < 'Ab aB..' < 'ab zz..' in chunk 0
    assert ref.ordered_ids('all', [b'ab', b'zz']).tolist() == [0, 3, 1, (1 << 32) | 1, 1 << 32]
    assert ref.ordered_ids('glob', b'*zz*ab*').tolist() == [0, 1 << 32, (1 << 32) | 1]    # driver zz: 'zz AB' < 'ZZ ab'; 'zz Ab zz ab'
    for kind, q in (('all', [b'ab', b'zz']), ('glob', b'*zz*ab*'), ('all', ([b'ab'], [b'zz']))):
        want = ref.search_all_ids(q) if kind == 'all' else ref.search_glob_ids(q)
        assert np.array_equal(np.sort(ref.ordered_ids(kind, q)), want)


# ---- the surface ---------------------------------------------------------------------------------------------------------

def test_the_six_symbols_are_declared_exported_and_mirrored():
    from pysubstringsearch_amd import _ffi
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32, pvp = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)
    for name in SYMBOLS:
        assert f'int {name}(' in hdr, name
        fn = getattr(_ffi.lib, name)
        last = vp if name.startswith('pss_reader_count') else pvp
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [vp, vp, vp, u32, vp, u32, vp, last]
        exact = getattr(_ffi.lib, name.replace('_icase', ''))
        assert list(exact.argtypes) == list(fn.argtypes)                # arguments exactly as the exact-byte namesake's


def test_the_keyword_is_on_all_ten_methods_and_in_the_stubs():
    import pysubstringsearch_amd as P
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in ALL_METHODS + GLOB_METHODS:
        # (the keyword sits on a functools.wraps wrapper around the exact-byte method, whose own signature is unchanged)
        method = getattr(P.Reader, name)
        assert 'icase' not in inspect.signature(method).parameters and 'icase' not in inspect.signature(method.__wrapped__).parameters
        par = inspect.signature(method, follow_wrapped=False).parameters['icase']
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False, name
        assert '``icase=True``' in method.__doc__ and method.__name__ == name
        line = next(ln for ln in stub.splitlines() if f'def {name}(' in ln)
        assert '*, icase: bool = False' in line, name


def test_c_abi_argument_errors_without_a_reader():
    """A malformed batch is reported as such with or without a reader; *out and counts stay untouched."""
    from pysubstringsearch_amd import _ffi
    blob, offs = b'abc', np.array([0, 2, 2, 3], dtype=np.uint64)
    goff, flags = np.array([0, 1, 3], dtype=np.uint64), np.zeros(3, dtype=np.uint8)
    for name in SYMBOLS:
        fn = getattr(_ffi.lib, name)
        noun = 'term' if '_terms_' in name else 'segment'
        if name.startswith('pss_reader_count'):
            sink = np.full(3, 7, dtype=np.uint64)
            assert fn(None, blob, offs.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, sink.ctypes.data) == _ffi.PSS_EINVAL
            assert sink.tolist() == [7, 7, 7]
        else:
            out = ctypes.c_void_p()
            assert fn(None, blob, offs.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
            assert not out.value
        assert f'{name}: {noun} 1 is empty' in _ffi.last_error()
        # a group without a member
        good = np.array([0, 1, 2, 3], dtype=np.uint64)
        bad_g = np.array([0, 3, 3], dtype=np.uint64)
        sink = np.full(3, 7, dtype=np.uint64)
        out = ctypes.c_void_p()
        last = sink.ctypes.data if name.startswith('pss_reader_count') else ctypes.byref(out)
        assert fn(None, blob, good.ctypes.data, 3, bad_g.ctypes.data, 2, flags.ctypes.data, last) == _ffi.PSS_EINVAL
        assert 'group 1 has no' in _ffi.last_error() and not out.value and sink.tolist() == [7, 7, 7]
        # a good batch and no reader
        assert fn(None, blob, good.ctypes.data, 3, goff.ctypes.data, 2, flags.ctypes.data, last) == _ffi.PSS_EINVAL
        assert 'no reader' in _ffi.last_error() and not out.value and sink.tolist() == [7, 7, 7]


class _NoDevice:
    """A Reader whose handle must never be asked for: the argument errors below are raised before the library is called."""

    def _handle(self):
        raise AssertionError('the library was called')


def _unbound(name):
    import pysubstringsearch_amd as P
    return lambda *a, **k: getattr(P.Reader, name)(_stub_reader(), *a, **k)


def _stub_reader():
    import pysubstringsearch_amd as P
    r = object.__new__(P.Reader)
    r._handle = _NoDevice()._handle
    return r


def test_python_argument_errors_need_no_device():
    for name in ALL_METHODS[:3]:
        call = _unbound(name)
        for bad in ([[b'']], [[b'ab', b'']], [([b'a'], [b''])]):
            with pytest.raises(ValueError, match='empty'):
                call(bad, icase=True)
        with pytest.raises(ValueError, match='no include term'):
            call([([], [b'a'])], icase=True)
        with pytest.raises(ValueError, match='no include term'):
            call([[]], icase=True)
        for bad in ([b'ab'], ['ab'], [['ab']], [[None]], b'ab'):
            with pytest.raises(TypeError):
                call(bad, icase=True)
        for flag in (1, 0, None, 'yes', b'x'):
            with pytest.raises(TypeError, match='icase'):
                call([[b'ab']], icase=flag)
        with pytest.raises(TypeError):
            call([[b'ab']], True)                                       # keyword-only
    for name in GLOB_METHODS[:3]:
        call = _unbound(name)
        for bad in ([b''], [b'*'], [b'**'], [b'ab', b'']):
            with pytest.raises(ValueError):
                call(bad, icase=True)
        for bad in (b'ab', 'ab', ['ab'], [None]):
            with pytest.raises(TypeError):
                call(bad, icase=True)
        for flag in (1, None, 'yes'):
            with pytest.raises(TypeError, match='icase'):
                call([b'ab'], icase=flag)
        with pytest.raises(TypeError):
            call([b'ab'], True)
    for name, args in (('search_all', (['a'],)), ('count_all', (['a'],)), ('search_glob', ('a',)), ('count_glob', ('a',))):
        call = _unbound(name)
        with pytest.raises(TypeError, match='icase'):
            call(*args, icase=1)
        with pytest.raises(TypeError):
            call(*args, True) if name.endswith('glob') else call(*args, (), True)
    for name in ('search_all', 'count_all'):
        with pytest.raises(ValueError):
            _unbound(name)([''], icase=True)
        with pytest.raises(TypeError):
            _unbound(name)('ab', icase=True)
    for name in ('search_glob', 'count_glob'):
        with pytest.raises(ValueError):
            _unbound(name)('*', icase=True)
        with pytest.raises(TypeError):
            _unbound(name)(b'ab', icase=True)
