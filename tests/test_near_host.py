"""The host side of the search within k mismatches (include/pss.h, pss_near_pieces and the argument checks of the three
pss_reader_*_near_* calls): no reader, no GPU.  A pattern of L > k bytes is cut into k + 1 non-empty pieces, piece j =
pattern[j L // (k + 1) : (j + 1) L // (k + 1)].  Beside the library's host code, the reference of tests/near_ref.py is
held against a second, independent statement of the contract (one regular expression per set of mismatch positions), and
the rule set the two kernels implement, restated hit by hit (near_ref.rule_set_lines), against the reference."""
import ctypes
import itertools
import os
import pathlib
import re

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi, near_pieces
from tests.near_ref import NearRef, pieces, rule_set_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGETS = range(0, 4)
C_CALLS = ('pss_reader_search_near_batch', 'pss_reader_search_near_ids_batch', 'pss_reader_count_near_batch')
METHODS = ('search_near_batch_packed', 'search_near_ids_batch', 'count_near_bytes', 'search_near', 'count_near')


# ---- near_pieces ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', BUDGETS)
def test_pieces_partition_every_pattern(k):
    rng = np.random.default_rng(1500 + k)
    for L in range(k + 1, 41):
        p = bytes(rng.integers(0, 256, L, dtype=np.uint8))
        got = near_pieces(p, k)
        assert len(got) == k + 1, (L, k)
        assert all(piece for _, piece in got), (L, k)                          # non-empty
        assert b''.join(piece for _, piece in got) == p                        # they concatenate to the pattern ...
        assert [off for off, _ in got] == list(itertools.accumulate([0] + [len(piece) for _, piece in got[:-1]]))      # ... at their offsets
        lens = [len(piece) for _, piece in got]
        assert max(lens) - min(lens) <= 1, (L, k, lens)
        assert got == [(j * L // (k + 1), p[j * L // (k + 1):(j + 1) * L // (k + 1)]) for j in range(k + 1)] == pieces(p, k)


def test_pieces_examples():
    assert near_pieces(b'password', 1) == [(0, b'pass'), (4, b'word')]
    assert near_pieces(b'password', 0) == [(0, b'password')]
    assert near_pieces(b'abab', 1) == [(0, b'ab'), (2, b'ab')] and near_pieces(b'aaaa', 3) == [(j, b'a') for j in range(4)]
    assert near_pieces(b'aabaa', 1) == [(0, b'aa'), (2, b'baa')]               # (nested pieces: `aa` inside `baa`)
    assert near_pieces(bytearray(b'a\x00\n\xff'), 3) == [(0, b'a'), (1, b'\x00'), (2, b'\n'), (3, b'\xff')]
    assert near_pieces(b'x' * 1000, 2) == [(0, b'x' * 333), (333, b'x' * 333), (666, b'x' * 334)]


def test_pieces_errors():
    with pytest.raises(ValueError, match='empty'):
        near_pieces(b'', 0)
    for p, k in ((b'a', 1), (b'ab', 2), (b'abc', 3), (b'ab', 3)):
        with pytest.raises(ValueError, match='every window'):
            near_pieces(p, k)
    for k in (4, 5, 255, -1, 1 << 40):
        with pytest.raises(ValueError, match='0 .. 3'):
            near_pieces(b'abcdefgh', k)
    for bad in ('abc', None, 5, [b'abc']):
        with pytest.raises(TypeError):
            near_pieces(bad, 1)
    for bad in (1.0, '1', None, True, b'1'):
        with pytest.raises(TypeError):
            near_pieces(b'abc', bad)
    lib = _ffi.lib
    off, ln, cnt = (ctypes.c_uint32 * 4)(7, 7, 7, 7), (ctypes.c_uint32 * 4)(7, 7, 7, 7), ctypes.c_uint32(7)
    assert lib.pss_near_pieces(b'', 0, 0, off, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL and 'empty' in _ffi.last_error()
    assert lib.pss_near_pieces(None, 3, 0, off, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert lib.pss_near_pieces(b'abcde', 5, 4, off, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL and '0 .. 3' in _ffi.last_error()
    assert lib.pss_near_pieces(b'abc', 3, 3, off, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL and 'every window' in _ffi.last_error()
    assert lib.pss_near_pieces(b'abc', 3, 1, None, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert lib.pss_near_pieces(b'abc', 3, 1, off, None, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert lib.pss_near_pieces(b'abc', 3, 1, off, ln, None) == _ffi.PSS_EINVAL
    assert list(off) == [7] * 4 and list(ln) == [7] * 4 and cnt.value == 7
    assert lib.pss_near_pieces(b'abcde', 5, 2, off, ln, ctypes.byref(cnt)) == _ffi.PSS_OK
    assert cnt.value == 3 and list(off) == [0, 1, 3, 7] and list(ln) == [1, 2, 2, 7]


# ---- the argument checks of the three calls, without a reader ---------------------------------------------------------------

def c_batch(patterns, offsets=None):
    blob = b''.join(patterns)
    offs = np.cumsum([0] + [len(t) for t in patterns]).astype(np.uint64) if offsets is None else np.array(offsets, dtype=np.uint64)
    return blob, offs


def test_einval_cases_with_a_null_reader():
    """Every malformed batch is reported as such without a reader; the null reader is judged last."""
    lib = _ffi.lib
    searches = (lib.pss_reader_search_near_batch, lib.pss_reader_search_near_ids_batch)

    def refused(what, blob, offs, nq, ks, out_ok=True):
        offs_p = None if offs is None else offs.ctypes.data
        ks = None if ks is None else np.array(ks, dtype=np.uint8)
        ks_p = None if ks is None else ks.ctypes.data
        for fn in searches:
            out = ctypes.c_void_p()
            assert fn(None, blob, offs_p, nq, ks_p, ctypes.byref(out) if out_ok else None) == _ffi.PSS_EINVAL
            assert not out.value and fn.__name__ in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())
        counts = np.full(4, 7, dtype=np.uint64)
        assert lib.pss_reader_count_near_batch(None, blob, offs_p, nq, ks_p, counts.ctypes.data if out_ok else None) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pss_reader_count_near_batch' in _ffi.last_error() and what in _ffi.last_error()

    blob, offs = c_batch([b'ab', b'', b'c'])
    refused('pattern 1 is empty', blob, offs, 3, [0, 0, 0])
    refused('pattern 0 is empty', *c_batch([b'']), 1, [0])
    blob, offs = c_batch([b'abcd', b'ab', b'abc'])
    refused('pattern 1 has 2 bytes and a budget of 2', blob, offs, 3, [3, 2, 2])
    refused('pattern 2 has 3 bytes and a budget of 3', blob, offs, 3, [0, 1, 3])
    refused('pattern 0 has a budget of 4 mismatches: 0 .. 3', blob, offs, 3, [4, 1, 1])
    refused('pattern 2 has a budget of 255', blob, offs, 3, [1, 1, 255])
    refused('start at 1, not at 0', *c_batch([b'ab', b'c'], [1, 2, 3]), 2, [0, 0])
    refused('decrease at pattern 1', *c_batch([b'abc', b'c'], [0, 3, 2]), 2, [0, 0])
    blob, offs = c_batch([b'ab', b'c'])
    refused('bad arguments', None, offs, 2, [1, 0])
    refused('bad arguments', blob, None, 2, [1, 0])
    refused('bad arguments', blob, offs, 2, None)
    refused('bad arguments', blob, offs, 2, [1, 0], out_ok=False)
    # a well-formed batch: the missing reader is what is left to report
    refused('no reader', blob, offs, 2, [1, 0])
    refused('no reader', *c_batch([b'Error\n', b'12', b'abcdefghijklmnopqrstuvwxyz' * 8]), 3, [3, 1, 2])
    refused('no reader', b'', np.zeros(1, dtype=np.uint64), 0, [])
    refused('no reader', b'', np.zeros(1, dtype=np.uint64), 0, None)


def test_python_argument_checks_need_no_reader():
    args = pss.Reader._near_args
    blob, offs, ks = args([b'password', b'ab'], 1)
    assert bytes(blob) == b'passwordab' and offs.tolist() == [0, 8, 10] and ks.dtype == np.uint8 and ks.tolist() == [1, 1]
    assert args([b'password', b'ab', bytearray(b'xyz1')], [3, 0, np.uint8(2)])[2].tolist() == [3, 0, 2]
    assert args([b'abc'], np.array([2]))[2].tolist() == [2] and args([], 3)[2].size == 0 and args([], [])[2].size == 0
    assert args([b'a', b'b'], 0)[2].tolist() == [0, 0]
    with pytest.raises(ValueError, match='pattern 1 is empty'):
        args([b'a', b''], 0)
    with pytest.raises(ValueError, match='pattern 1 has 2 bytes and a budget of 2'):
        args([b'abc', b'ab'], 2)
    with pytest.raises(ValueError, match='pattern 0 has 1 bytes and a budget of 1'):
        args([b'a', b'abcd'], [1, 3])
    for bad in (4, -1, [1, 4], [0, 256]):
        with pytest.raises(ValueError, match='0 .. 3'):
            args([b'abcdefgh', b'abcdefgh'], bad)
    for bad in ([1], [1, 1, 1], []):
        with pytest.raises(ValueError, match='budgets for 2 patterns'):
            args([b'abcdefgh', b'abcdefgh'], bad)
    for bad in (1.0, None, '1', b'1', True, [1, 1.5], [1, None], [True, 1]):
        with pytest.raises(TypeError):
            args([b'abcdefgh', b'abcdefgh'], bad)
    for bad in (b'ab', 'ab', ['ab'], [None]):
        with pytest.raises(TypeError):
            args(bad, 1)


# ---- declarations -----------------------------------------------------------------------------------------------------

def test_declarations():
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for name in C_CALLS + ('pss_near_pieces',):
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    assert list(_ffi.lib.pss_reader_search_near_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_near_ids_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_near_batch.argtypes) == [vp, vp, vp, u32, vp, vp]
    assert list(_ffi.lib.pss_near_pieces.argtypes) == [vp, u64, u32] + [ctypes.POINTER(u32)] * 3
    # the contract is written out in the header, the limits among it
    for phrase in ('INSIDE THE\n * ENTRY', 'k > 3', 'insertions and deletions', 'FIRST\n * exact piece', 'LEFTMOST near match'):
        assert phrase in hdr, phrase
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in METHODS + ('near_pieces',):
        assert f'def {name}(' in stub, f'{name} is missing from __init__.pyi'
    assert 'near_pieces' in pss.__all__
    for name in METHODS:
        doc = getattr(pss.Reader, name).__doc__
        assert doc and '``k' in doc, name
    from pysubstringsearch_amd import dist
    assert not any('near' in name for name in dir(dist.ShardedReader))         # (stated as not built)
    # no route bit and no environment switch of its own
    assert not any('NEAR' in name for name in _ffi.ROUTES) and 'PSS_ROUTE_NEAR' not in hdr and 'PSS_NEAR' not in hdr


# ---- the reference against a second statement of the contract ------------------------------------------------------------------

def regex_lines(text: bytes, pattern: bytes, k: int):
    """Lines of text (entries closed by 0x0A, or the unterminated rest) that hold pattern within k mismatches: per set of
    at most k positions, the pattern with those positions replaced by `any byte but a newline`, searched line by line."""
    if b'\n' in pattern:
        return []
    lines = text.split(b'\n')
    if text.endswith(b'\n') or not text:
        lines = lines[:-1]
    L, rx = len(pattern), []
    for r in range(k + 1):
        for at in itertools.combinations(range(L), r):
            rx.append(re.compile(b''.join(b'[^\n]' if i in at else re.escape(pattern[i:i + 1]) for i in range(L)), re.DOTALL))
    return [i for i, ln in enumerate(lines) if any(x.search(ln) for x in rx)]


TEXTS = [b'password\npassw0rd\npa55word\npassword1\nassword\npasswor\n\npass\nword\np@ssw0rd\np@ssw0r\nd',
         b'ab\ncd\nabZcd\nab\ncdx\nabab\nabba\nbaab\n',
         b'aaaa\naaa\nbaaa\nabab\nbbbb\naabb',
         b'\x00\x00a\xff\n\xff\xfe\x00\n\x00\n',
         b'', b'\n', b'x', b'abcabcabcabdabcabc\nabcabdabcabc\n']
PATTERNS = [(b'password', 0), (b'password', 1), (b'password', 2), (b'password', 3), (b'abZcd', 1), (b'abXcd', 1), (b'abcd', 1), (b'abab', 1),
            (b'aaaa', 3), (b'aaaa', 1), (b'aab', 1), (b'a', 0), (b'ab', 1), (b'\x00\x00', 1), (b'\xff\xfe\x00', 2), (b'a\x00', 1), (b'ab\ncd', 1),
            (b'abcabc', 2), (b'x', 0), (b'xy', 1)]


def test_the_reference_agrees_with_a_regex_per_mismatch_set():
    ref = NearRef(TEXTS)
    some = 0
    for p, k in PATTERNS:
        want = [(c << 32) | line for c, t in enumerate(TEXTS) for line in regex_lines(t, p, k)]
        got = ref.search_near_ids(p, k).tolist()
        assert got == want, (p, k)
        assert sorted(ref.ordered_ids(p, k).tolist()) == got
        some += len(got)
    assert some > 60
    # the window lies inside the entry: `ab\ncd` is no match for abZcd, in either entry
    assert ref.search_near_ids(b'abZcd', 1).tolist() == [(1 << 32) | 2]
    assert ref.search_near_ids(b'ab\ncd', 1).size == 0 and ref.piece_hits(b'ab\ncd', 1) == 0
    # the unterminated last entry's last byte takes part
    assert (0 << 32) | 11 not in ref.search_near_ids(b'dd', 0).tolist() and ((0 << 32) | 11) in ref.search_near_ids(b'd', 0).tolist()
    assert ref.piece_hits(b'abab', 1) == 2 * sum(t.count(b'ab') for t in TEXTS)


def test_the_rule_set_of_the_kernels_agrees_with_the_reference():
    """Piece hits, the five steps of the hit verify and the leftward dedupe, restated on the CPU, keep exactly one hit per
    matching entry and leave them in the stated order: 1 500 random small cases over alphabets of 2 - 4 letters, with
    repeated and nested pieces and windows across newlines among them."""
    rng = np.random.default_rng(1510)
    matched = crossing = repeated = 0
    for _ in range(1500):
        sigma = int(rng.integers(2, 5))
        abc = np.frombuffer(b'abcd'[:sigma] + b'\n', np.uint8)
        pr = np.r_[np.full(sigma, 1.0), 0.12 * sigma]
        text = bytes(abc[rng.choice(sigma + 1, int(rng.integers(1, 60)), p=pr / pr.sum())])
        k = int(rng.integers(0, 4))
        p = bytes(abc[rng.integers(0, sigma, int(rng.integers(k + 1, k + 8)))])
        ref = NearRef([text])
        want = ref.ordered_ids(p, k).tolist()
        assert rule_set_lines(text, p, k) == want, (text, p, k)
        assert sorted(want) == ref.search_near_ids(p, k).tolist()
        matched += len(want)
        t, q = np.frombuffer(text, np.uint8), np.frombuffer(p, np.uint8)
        crossing += any(0x0A in text[s:s + len(p)] and int((t[s:s + len(p)] != q).sum()) <= k for s in range(len(text) - len(p) + 1))
        repeated += len({piece for _, piece in pieces(p, k)}) <= k
    assert matched > 1500 and crossing > 200 and repeated > 300, (matched, crossing, repeated)
