"""The wildcard search without a GPU: the brute-force reference of tests/glob_ref.py against hand-written cases (so the
yardstick of tests/test_glob_gpu.py is itself pinned) and against an independent check -- recursive backtracking over
bytes.find, no regular expression -- over random texts; glob_parse / glob_escape; then the surface -- the three C entry
points are exported and bound, no route bit and no struct size was added, the Reader has the methods and the stubs name
them, and bad batches are refused before any device is touched."""
import ctypes
import os
import pathlib

import numpy as np
import pytest

from tests.glob_ref import END, START, GlobRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pss_reader_search_seq_batch', 'pss_reader_search_seq_ids_batch', 'pss_reader_count_seq_batch')
METHODS = ('search_glob_batch_packed', 'search_glob_ids_batch', 'count_glob_bytes', 'search_glob', 'count_glob')


# ---- the reference ---------------------------------------------------------------------------------------------------

def test_reference_on_hand_written_cases():
    #        0              1              2  3   4    5     6      7    8
    text = b'error timeout\ntimeout error\na\naa\naba\nabba\nabxba\nxaay\n\n'
    ref = GlobRef([text])
    ids = lambda segs, anch=0: ref.search_seq_ids(segs, anch).tolist()
    assert ids([b'error', b'timeout']) == [0] and ids([b'timeout', b'error']) == [1]      # order matters
    assert ids([b'error']) == [0, 1] and ids([b'r', b'r', b'r']) == [0, 1]
    assert ids([b'a', b'a']) == [3, 4, 5, 6, 7]                                           # a*a does not match 'a'
    assert ids([b'a', b'a'], START | END) == [3, 4, 5, 6] and ids([b'a'], START | END) == [2]
    assert ids([b'ab', b'ba']) == [5, 6] and ids([b'ab', b'ba'], START | END) == [5, 6]   # not 'aba': no overlap
    assert ids([b'a', b'a', b'a']) == [] and ids([b'a', b'a', b'a'], START | END) == []   # *a*a*a* needs three
    assert GlobRef([b'banana\naa\n']).search_seq_ids([b'a', b'a', b'a'], 0).tolist() == [0]
    # the four anchor combinations of one pair of segments
    assert ids([b'a', b'y']) == [7] and ids([b'a', b'y'], START) == [] and ids([b'a', b'y'], END) == [7] and ids([b'x', b'y'], START | END) == [7]
    assert ids([b'x', b'a'], START) == [7] and ids([b'x', b'a'], START | END) == [] and ids([b'x', b'a'], END) == [6]
    assert ids([b'e', b't'], START) == [0] and ids([b'e', b't'], END) == [0] and ids([b't', b'r'], START | END) == [1]
    # one segment, both anchors: equality
    assert ids([b'aba'], START | END) == [4] and ids([b'ab'], START | END) == [] and ids([b'ab'], START) == [4, 5, 6] and ids([b'ba'], END) == [4, 5, 6]
    # a newline segment matches nothing, although bytes.find sees it in the text
    assert text.find(b'a\naa') >= 0
    assert ids([b'a\naa']) == [] and ids([b'\n']) == [] and ids([b'a', b'\n'], START) == [] and ids([b'a', b'a\n']) == []


def test_reference_on_chunk_edges_and_file_indexes():
    # chunk 4: the entry at offset 0, an empty entry; chunk 7: no closing newline, 'ab' ends at the very last byte
    ref = GlobRef([b'ab x\n\nx ab\n', b'x\nab\nx ab'], indices=[4, 7])
    a, c = 4 << 32, 7 << 32
    assert ref.search_seq_ids([b'x', b'b'], 0).tolist() == [a | 2, c | 2]
    assert ref.search_seq_ids([b'x', b'ab'], START | END).tolist() == [a | 2, c | 2]       # the last byte takes part
    assert ref.search_seq_ids([b'a'], END).tolist() == [] and ref.search_seq_ids([b'b'], END).tolist() == [a | 2, c | 1, c | 2]
    assert ref.entry(c | 2) == b'x a'                                                       # ... though the text handed out loses it
    assert ref.search_seq_ids([b'ab', b'x'], START).tolist() == [a]
    assert ref.search_seq_ids([b'b', b'\x00'], 0).tolist() == []
    assert GlobRef([b'']).search_seq_ids([b'a'], 0).size == 0 and GlobRef([b'a']).search_seq_ids([b'a'], START | END).tolist() == [0]
    assert ref.search_glob_ids(b'x*ab').tolist() == [a | 2, c | 2] and ref.search_glob_ids(b'*b*x*').tolist() == [a]


def backtrack(entry: bytes, segments, anchors: int) -> bool:
    """Does entry match?  Every occurrence of every segment is tried, by bytes.find alone."""
    def place(j: int, lo: int) -> bool:
        if j == len(segments):
            return True
        s, p = segments[j], entry.find(segments[j], lo)
        while p >= 0:
            first_ok = j > 0 or not anchors & START or p == 0
            last_ok = j < len(segments) - 1 or not anchors & END or p + len(s) == len(entry)
            if first_ok and last_ok and place(j + 1, p + len(s)):
                return True
            p = entry.find(s, p + 1)
        return False
    return place(0, 0)


def test_reference_agrees_with_backtracking_over_random_texts():
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b'ab\n', np.uint8)
    pieces = [b'a', b'b', b'ab', b'ba', b'aa', b'aba', b'bab', b'abab', b'bb']
    seen = set()
    for _ in range(60):
        n = int(rng.integers(1, 120))
        text = bytes(alphabet[rng.choice(3, n, p=[0.45, 0.35, 0.2])])
        lines = text.split(b'\n')
        if text.endswith(b'\n'):
            lines.pop()                       # (the text ends with a terminated entry, not with an empty unterminated one)
        ref = GlobRef([text])
        for _ in range(16):
            segs = [pieces[int(i)] for i in rng.integers(0, len(pieces), int(rng.integers(1, 5)))]
            anch = int(rng.integers(0, 4))
            want = [i for i, ln in enumerate(lines) if backtrack(ln, segs, anch)]
            assert ref.search_seq_ids(segs, anch).tolist() == want, (text, segs, anch)
            seen.add((anch, bool(want)))
    assert len(seen) == 8                     # every anchor combination both matched and missed


# ---- glob_parse / glob_escape ------------------------------------------------------------------------------------------

def test_glob_parse():
    from pysubstringsearch_amd import glob_parse
    assert glob_parse(b'abc') == ([b'abc'], START | END)
    assert glob_parse(b'*abc*') == ([b'abc'], 0) and glob_parse(b'abc*') == ([b'abc'], START) and glob_parse(b'*abc') == ([b'abc'], END)
    assert glob_parse(b'GET */admin* 500') == ([b'GET ', b'/admin', b' 500'], START | END)
    assert glob_parse(b'*a*b*c*') == ([b'a', b'b', b'c'], 0)
    assert glob_parse(b'**a***b**') == ([b'a', b'b'], 0) and glob_parse(b'a**b') == ([b'a', b'b'], START | END)      # ** collapses
    assert glob_parse(rb'a\*b') == ([b'a*b'], START | END) and glob_parse(rb'a\\b') == ([b'a\\b'], START | END)
    assert glob_parse(rb'a\\*b') == ([b'a\\', b'b'], START | END)                   # an escaped backslash, then a wildcard
    assert glob_parse(rb'\*a*') == ([b'*a'], START) and glob_parse(rb'*a\*') == ([b'a*'], END)     # \* at an end is a literal: anchored
    assert glob_parse(rb'\*') == ([b'*'], START | END) and glob_parse(rb'*\**') == ([b'*'], 0)
    assert glob_parse(rb'\a\b') == ([b'ab'], START | END)                           # any byte may be escaped
    assert glob_parse(b'a\nb*\x00') == ([b'a\nb', b'\x00'], START | END)            # no byte is special but * and \
    assert glob_parse(bytearray(b'a*')) == ([b'a'], START)
    for bad in (b'', b'*', b'**', b'***'):
        with pytest.raises(ValueError, match='no literal byte.*entry_counts.*search_exact'):
            glob_parse(bad)
    for bad in (b'\\', b'a\\', rb'a*\\' + b'\\', b'*\\'):
        with pytest.raises(ValueError, match='lone backslash'):
            glob_parse(bad)
    with pytest.raises(TypeError):
        glob_parse('a*b')


def test_glob_escape_round_trip():
    from pysubstringsearch_amd import glob_escape, glob_parse
    assert glob_escape(b'a*b\\c') == rb'a\*b\\c' and glob_escape(b'plain') == b'plain' and glob_escape(b'') == b''
    rng = np.random.default_rng(12)
    pool = np.array([b for b in range(256) if b != 0x0A], dtype=np.uint8)
    weights = np.where((pool == 0x2A) | (pool == 0x5C), 40.0, 1.0)
    for _ in range(300):
        x = bytes(pool[rng.choice(pool.size, int(rng.integers(1, 24)), p=weights / weights.sum())])
        assert glob_parse(glob_escape(x)) == ([x], START | END), x
        assert glob_parse(b'*' + glob_escape(x) + b'*' + glob_escape(x)) == ([x, x], END)
    with pytest.raises(TypeError):
        glob_escape('a')


# ---- the surface -----------------------------------------------------------------------------------------------------

def test_library_exports_and_binding_declares_the_entry_points():
    from pysubstringsearch_amd import _ffi
    raw = ctypes.CDLL(os.path.join(ROOT, 'pysubstringsearch_amd', 'libpss.so'))
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in SYMBOLS:
        assert hasattr(raw, name), f'{name} is not exported by libpss.so'
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        assert getattr(_ffi.lib, name).restype is ctypes.c_int
    assert list(_ffi.lib.pss_reader_search_seq_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_seq_ids_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_seq_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, vp]
    assert (_ffi.ANCHOR_START, _ffi.ANCHOR_END) == (START, END) == (_ffi.ANCHORS['start'], _ffi.ANCHORS['end'])


def test_no_route_bit_and_no_struct_size_was_added():
    from pysubstringsearch_amd import _ffi
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    assert hdr.count('#define PSS_ROUTE_') == len(_ffi.ROUTES) == 14
    assert max(_ffi.ROUTES.values()) == _ffi.ROUTES['ANCHORED'] == 0x2000
    assert _ffi.lib.pss_search_stats_size() == ctypes.sizeof(_ffi.SearchStats) == 64


def test_reader_has_the_methods_and_the_stubs_name_them():
    import inspect

    import pysubstringsearch_amd as P
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in METHODS:
        assert hasattr(P.Reader, name), name
        assert f'def {name}(' in stub, f'{name} is missing from __init__.pyi'
    for name in METHODS[:3]:
        assert list(inspect.signature(getattr(P.Reader, name)).parameters) == ['self', 'patterns']
    for name in METHODS[3:]:
        assert list(inspect.signature(getattr(P.Reader, name)).parameters) == ['self', 's']
    for name in ('glob_parse', 'glob_escape'):
        assert name in P.__all__ and callable(getattr(P, name)) and f'def {name}(' in stub


def test_patterns_are_packed_for_the_library():
    import pysubstringsearch_amd as P
    blob, offs, goff, anch = P.Reader._glob_args([b'ab*c', b'*x*yz*ab', rb'q\*'])
    assert blob == b'abcxyzabq*' and offs.tolist() == [0, 2, 3, 4, 6, 8, 10]
    assert goff.tolist() == [0, 2, 5, 6] and goff.dtype == np.uint64
    assert anch.tolist() == [3, 2, 3] and anch.dtype == np.uint8
    blob, offs, goff, anch = P.Reader._glob_args([])
    assert blob == b'' and offs.tolist() == [0] and goff.tolist() == [0] and anch.size >= 1
    r = P.Reader._from_handle(ctypes.c_void_p())
    with pytest.raises(ValueError, match='closed Reader'):
        r.count_glob_bytes([b'a*b'])


def test_bad_patterns_are_refused_before_the_library_is_called():
    import pysubstringsearch_amd as P
    r = P.Reader._from_handle(ctypes.c_void_p())      # (closed: reaching the library would raise 'closed Reader' instead)
    calls = (r.search_glob_batch_packed, r.search_glob_ids_batch, r.count_glob_bytes)
    for call in calls:
        for bad, what in (([b'a', b'*'], 'no literal byte'), ([b''], 'no literal byte'), ([b'a\\'], 'lone backslash')):
            with pytest.raises(ValueError, match=what):
                call(bad)
        for bad in (b'a*b', 'a*b', bytearray(b'a*b'), ['a*b'], [[b'a', b'b']]):     # a bare pattern is not a sequence of them
            with pytest.raises(TypeError):
                call(bad)
    for bad in (b'a*b', [b'a*b'], ['a*b'], None):
        with pytest.raises(TypeError):
            r.search_glob(bad)
        with pytest.raises(TypeError):
            r.count_glob(bad)
    with pytest.raises(ValueError, match='no literal byte'):
        r.search_glob('*')
    with pytest.raises(ValueError, match='no literal byte'):
        r.count_glob('')


def c_batch(segs, goff, anch):
    blob = b''.join(segs)
    offs = np.cumsum([0] + [len(t) for t in segs]).astype(np.uint64)
    return blob, offs, np.array(goff, dtype=np.uint64), np.array(anch if anch else [0], dtype=np.uint8)


BAD_C_BATCHES = [
    ('no segment', [b'a', b'b'], [0, 0, 2], [0, 0]),               # an empty group
    ('no segment', [b'a'], [0, 1, 1], [3, 3]),
    ('is empty', [b'a', b''], [0, 2], [0]),
    ('is empty', [b'', b'a'], [0, 1, 2], [1, 2]),
    ('anchors[0] = 4', [b'a', b'b'], [0, 2], [4]),
    ('anchors[1] = 255', [b'a', b'b'], [0, 1, 2], [3, 255]),
    ('group offsets', [b'a', b'b'], [1, 2], [0]),                  # does not start at 0
    ('group offsets', [b'a', b'b'], [0, 1], [0]),                  # does not end at nsegs
    ('group offsets', [b'a', b'b', b'c'], [0, 2, 1, 3], [0, 0, 0]),      # decreases
    ('group offsets', [b'a', b'b'], [0, 3, 2], [0, 0]),            # passes nsegs
]


@pytest.mark.parametrize('what,segs,goff,anch', BAD_C_BATCHES)
def test_bad_batches_are_refused_by_the_c_calls(what, segs, goff, anch):
    """PSS_EINVAL with a message, *out and counts untouched.  The batch is judged before the reader is, so no device is
    needed; tests/test_glob_gpu.py repeats the calls on a live reader."""
    from pysubstringsearch_amd import _ffi
    blob, offs, g, a = c_batch(segs, goff, anch)
    ng = len(goff) - 1
    for fn in (_ffi.lib.pss_reader_search_seq_batch, _ffi.lib.pss_reader_search_seq_ids_batch):
        out = ctypes.c_void_p()
        assert fn(None, blob, offs.ctypes.data, len(segs), g.ctypes.data, ng, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert not out.value and what in _ffi.last_error(), _ffi.last_error()
    counts = np.full(4, 7, dtype=np.uint64)
    assert _ffi.lib.pss_reader_count_seq_batch(None, blob, offs.ctypes.data, len(segs), g.ctypes.data, ng, a.ctypes.data,
                                               counts.ctypes.data) == _ffi.PSS_EINVAL
    assert counts.tolist() == [7] * 4 and what in _ffi.last_error()


def test_null_arguments_are_refused_with_a_status():
    from pysubstringsearch_amd import _ffi
    blob, offs, g, a = c_batch([b'a', b'b'], [0, 2], [3])
    out = ctypes.c_void_p()
    args = (blob, offs.ctypes.data, 2, g.ctypes.data, 1, a.ctypes.data)
    assert _ffi.lib.pss_reader_search_seq_batch(None, *args, ctypes.byref(out)) == _ffi.PSS_EINVAL       # a good batch, no reader
    assert 'pss_reader_search_seq_batch' in _ffi.last_error() and 'no reader' in _ffi.last_error()
    assert _ffi.lib.pss_reader_search_seq_ids_batch(None, *args, None) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_count_seq_batch(None, *args, None) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_seq_batch(None, blob, offs.ctypes.data, 2, None, 1, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_seq_batch(None, blob, offs.ctypes.data, 2, g.ctypes.data, 1, None, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_seq_batch(None, blob, None, 2, g.ctypes.data, 1, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_seq_batch(None, None, offs.ctypes.data, 2, g.ctypes.data, 1, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert 'no reader' not in _ffi.last_error()
    assert not out.value
