"""The host side of the search within k edits (include/pss.h, the three pss_reader_*_edit_* calls): no
reader, no GPU.  The reference of tests/edit_ref.py -- a Sellers scan per entry -- is held against a second, independent
statement of the contract (the Levenshtein distance of every substring, by the textbook recursion), and the rule set the
kernels implement, restated hit by hit (edit_ref.rule_set_lines), against the reference.  Then the argument checks of the C
calls without a reader and of the Python layer without a device, and the declarations."""
import ctypes
import functools
import os
import pathlib

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi
from tests.edit_ref import EditRef, rule_set_lines, sellers
from tests.near_ref import NearRef, pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_CALLS = ('pss_reader_search_edit_batch', 'pss_reader_search_edit_ids_batch', 'pss_reader_count_edit_batch')
METHODS = ('search_near_batch_packed', 'search_near_ids_batch', 'count_near_bytes', 'search_near', 'count_near')


def lev(a: bytes, b: bytes) -> int:
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j - 1) + (a[i - 1] != b[j - 1]), d(i - 1, j) + 1, d(i, j - 1) + 1)
    return d(len(a), len(b))


def substring_distance(entry: bytes, pattern: bytes) -> int:
    return min(lev(entry[i:j], pattern) for i in range(len(entry) + 1) for j in range(i, len(entry) + 1))


def test_the_sellers_scan_is_the_least_distance_of_a_substring():
    rng = np.random.default_rng(1700)
    assert lev(b'kitten', b'sitting') == 3 and lev(b'', b'abc') == 3 and lev(b'abc', b'abc') == 0
    for _ in range(300):
        abc = np.frombuffer(b'abc'[:int(rng.integers(2, 4))], np.uint8)
        e = bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 12)))])
        p = bytes(abc[rng.integers(0, len(abc), int(rng.integers(1, 8)))])
        assert sellers(e, p) == substring_distance(e, p), (e, p)
    for e, p, want in ((b'pasword', b'password', 1), (b'passsword', b'password', 1), (b'passw0rd', b'password', 1), (b'my pass-word!', b'password', 1),
                       (b'psswrd', b'password', 2), (b'', b'abc', 3), (b'xxabcxx', b'abc', 0), (b'drowssap', b'password', 6)):
        assert sellers(e, p) == want, (e, p)


def test_the_rule_set_of_the_kernels_agrees_with_the_reference():
    """Piece hits, the two sides of every candidate, the earlier piece at the same place and the leftward dedupe, restated on
    the CPU, keep exactly one hit per matching entry and leave them in the stated order: 1 600 random small cases over
    alphabets of 2 and 3 letters and every k, newlines inside the text, repeated pieces (`abab`) and nested ones (`aab`)
    among them.  Beside it: the edit answer contains the Hamming answer, and k = 0 is the exact answer."""
    rng = np.random.default_rng(1710)
    matched = more = repeated = nested = walled = 0
    fixed = [(b'abab\nabb\nbab\naab\nab\n', b'abab', 1), (b'aab\nab\naa\nb\nabaab', b'aab', 1), (b'ab\nab\n', b'abab', 1), (b'a\nb', b'ab', 1)]
    for i in range(1600):
        if i < len(fixed):
            text, p, k = fixed[i]
        else:
            sigma = int(rng.integers(2, 4))
            abc = np.frombuffer(b'abc'[:sigma] + b'\n', np.uint8)
            pr = np.r_[np.full(sigma, 1.0), 0.15 * sigma]
            text = bytes(abc[rng.choice(sigma + 1, int(rng.integers(1, 48)), p=pr / pr.sum())])
            k = int(rng.integers(0, 4))
            p = bytes(abc[rng.integers(0, sigma, int(rng.integers(k + 1, 10)))])
        ref, near = EditRef([text]), NearRef([text])
        want = ref.ordered_ids(p, k).tolist()
        assert rule_set_lines(text, p, k) == want, (text, p, k)
        ids = ref.search_edit_ids(p, k).tolist()
        assert sorted(want) == ids and len(set(want)) == len(want)
        hamming = near.search_near_ids(p, k).tolist()
        assert set(hamming) <= set(ids), (text, p, k)
        if k == 0:
            assert ids == hamming == [line for line, e in enumerate(ref._true[0]) if p in e]
        matched += len(ids)
        more += len(ids) > len(hamming)
        cut = [piece for _, piece in pieces(p, k)]
        repeated += len(set(cut)) <= k
        nested += any(a != b and b.startswith(a) for a in cut for b in cut)
        # a match that would need the newline among its edits: the joined neighbours hold the pattern, neither of them does
        lines = text.split(b'\n')
        walled += any(sellers(a + b, p) <= max(k - 1, 0) and sellers(a, p) > k and sellers(b, p) > k for a, b in zip(lines, lines[1:]))
    assert matched > 1500 and more > 300 and repeated > 300 and nested > 100 and walled > 30, (matched, more, repeated, nested, walled)


def test_examples_of_the_contract():
    text = b'password\npasword\npasssword\npassw0rd\npass-word\npass\nword\npsswrd\nmy pasword!\ndrowssap'
    ref = EditRef([text])
    assert ref.search_edit_ids(b'password', 0).tolist() == [0]
    assert ref.search_edit_ids(b'password', 1).tolist() == [0, 1, 2, 3, 4, 8]
    assert ref.search_edit_ids(b'password', 2).tolist() == [0, 1, 2, 3, 4, 7, 8]
    assert NearRef([text]).search_near_ids(b'password', 1).tolist() == [0, 3]
    # never over a newline: `pass\nword` would be one deletion away
    assert 5 not in ref.search_edit_ids(b'password', 3).tolist() and 6 not in ref.search_edit_ids(b'password', 3).tolist()
    assert ref.search_edit_ids(b'pass\nword', 1).size == 0 and ref.piece_hits(b'pass\nword', 1) == 0
    assert ref.piece_hits(b'password', 1) == text.count(b'pass') + text.count(b'word')
    # the kept candidate: the smallest d, then the smallest j
    assert rule_set_lines(b'aab\n', b'aab', 1) == [0] and rule_set_lines(b'abab\n', b'abab', 1) == [0]


# ---- the argument checks of the three calls, without a reader ---------------------------------------------------------------

def c_batch(patterns, offsets=None):
    blob = b''.join(patterns)
    offs = np.cumsum([0] + [len(t) for t in patterns]).astype(np.uint64) if offsets is None else np.array(offsets, dtype=np.uint64)
    return blob, offs


def test_einval_cases_with_a_null_reader():
    """Every malformed batch is reported as such without a reader; the null reader is judged last."""
    lib = _ffi.lib
    searches = (lib.pss_reader_search_edit_batch, lib.pss_reader_search_edit_ids_batch)

    def refused(what, blob, offs, nq, ks, out_ok=True):
        offs_p = None if offs is None else offs.ctypes.data
        ks = None if ks is None else np.array(ks, dtype=np.uint8)
        ks_p = None if ks is None else ks.ctypes.data
        for fn in searches:
            out = ctypes.c_void_p()
            assert fn(None, blob, offs_p, nq, ks_p, ctypes.byref(out) if out_ok else None) == _ffi.PSS_EINVAL
            assert not out.value and fn.__name__ in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())
        counts = np.full(4, 7, dtype=np.uint64)
        assert lib.pss_reader_count_edit_batch(None, blob, offs_p, nq, ks_p, counts.ctypes.data if out_ok else None) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pss_reader_count_edit_batch' in _ffi.last_error() and what in _ffi.last_error()

    blob, offs = c_batch([b'ab', b'', b'c'])
    refused('pattern 1 is empty', blob, offs, 3, [0, 0, 0])
    blob, offs = c_batch([b'abcd', b'ab', b'abc'])
    refused('pattern 1 has 2 bytes and a budget of 2 edits: deleting all of it', blob, offs, 3, [3, 2, 2])
    refused('pattern 2 has 3 bytes and a budget of 3 edits', blob, offs, 3, [0, 1, 3])
    refused('pattern 0 has a budget of 4 edits: 0 .. 3', blob, offs, 3, [4, 1, 1])
    refused('pattern 2 has a budget of 255 edits', blob, offs, 3, [1, 1, 255])
    refused('start at 1, not at 0', *c_batch([b'ab', b'c'], [1, 2, 3]), 2, [0, 0])
    refused('decrease at pattern 1', *c_batch([b'abc', b'c'], [0, 3, 2]), 2, [0, 0])
    blob, offs = c_batch([b'ab', b'c'])
    refused('bad arguments', None, offs, 2, [1, 0])
    refused('bad arguments', blob, None, 2, [1, 0])
    refused('bad arguments', blob, offs, 2, None)
    refused('bad arguments', blob, offs, 2, [1, 0], out_ok=False)
    refused('no reader', blob, offs, 2, [1, 0])
    refused('no reader', *c_batch([b'Error\n', b'12', b'abcdefghijklmnopqrstuvwxyz' * 8]), 3, [3, 1, 2])
    refused('no reader', b'', np.zeros(1, dtype=np.uint64), 0, [])
    # the near calls keep their wording
    out = ctypes.c_void_p()
    blob, offs = c_batch([b'ab'])
    ks = np.array([2], dtype=np.uint8)
    assert lib.pss_reader_search_near_batch(None, blob, offs.ctypes.data, 1, ks.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert 'a budget of 2 mismatches: every window of its length matches it' in _ffi.last_error()


def test_python_argument_checks_need_no_reader():
    args = pss.Reader._near_args
    blob, offs, ks = args([b'password', b'ab'], 1, True)
    assert bytes(blob) == b'passwordab' and offs.tolist() == [0, 8, 10] and ks.dtype == np.uint8 and ks.tolist() == [1, 1]
    assert args([b'password', b'ab', bytearray(b'xyz1')], [3, 0, np.uint8(2)], edits=True)[2].tolist() == [3, 0, 2]
    assert args([], 3, True)[2].size == 0
    with pytest.raises(ValueError, match='pattern 1 is empty'):
        args([b'a', b''], 0, True)
    with pytest.raises(ValueError, match='pattern 1 has 2 bytes and a budget of 2 edits: deleting all of it'):
        args([b'abc', b'ab'], 2, True)
    with pytest.raises(ValueError, match='pattern 1 has 2 bytes and a budget of 2 mismatches: every window'):
        args([b'abc', b'ab'], 2)
    for bad in (4, -1, [1, 4], [0, 256]):
        with pytest.raises(ValueError, match='0 .. 3'):
            args([b'abcdefgh', b'abcdefgh'], bad, True)
    for bad in ([1], [1, 1, 1], []):
        with pytest.raises(ValueError, match='budgets for 2 patterns'):
            args([b'abcdefgh', b'abcdefgh'], bad, True)
    for bad in (1.0, None, '1', b'1', True, [1, 1.5]):
        with pytest.raises(TypeError):
            args([b'abcdefgh', b'abcdefgh'], bad, True)
    for bad in (1, 0, None, 'yes', [True]):
        with pytest.raises(TypeError, match='edits'):
            args([b'abcdefgh'], 1, bad)


def test_declarations():
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in C_CALLS:
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    assert list(_ffi.lib.pss_reader_search_edit_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_edit_ids_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_edit_batch.argtypes) == [vp, vp, vp, u32, vp, vp]
    for phrase in ('INSERTED,\n * DELETED or SUBSTITUTED', 'lc + rc <= k', 'never reaches over a newline', 'a transposition as one\n * edit'):
        assert phrase in hdr, phrase
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    import inspect
    for name in METHODS:
        assert 'edits: bool = False' in next(ln for ln in stub.splitlines() if f'def {name}(' in ln), name
        sig = inspect.signature(getattr(pss.Reader, name))
        assert sig.parameters['edits'].default is False, name
        assert 'edits=True' in getattr(pss.Reader, name).__doc__, name
    # no route bit and no environment switch of its own
    assert not any('EDIT' in name for name in _ffi.ROUTES) and 'PSS_ROUTE_EDIT' not in hdr and 'PSS_EDIT' not in hdr
