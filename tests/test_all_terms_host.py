"""The all-terms search without a GPU: the brute-force reference of tests/all_terms_ref.py against hand-written cases (so
the yardstick of tests/test_all_terms_gpu.py is itself pinned) and against set operations over the lines of random texts;
then the surface -- the three C entry points are exported and bound, no route bit and no struct size was added, the
Reader has the methods and the stubs name them, and bad batches are refused before any device is touched."""
import ctypes
import os
import pathlib

import numpy as np
import pytest

from tests.all_terms_ref import AllTermsRef, split_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pss_reader_search_terms_batch', 'pss_reader_search_terms_ids_batch', 'pss_reader_count_terms_batch')
METHODS = ('search_all_batch_packed', 'search_all_ids_batch', 'count_all_bytes', 'search_all', 'count_all')


# ---- the reference ---------------------------------------------------------------------------------------------------

def test_reference_on_hand_written_cases():
    #        0           1         2         3      4      5    6       7
    text = b'error timeout\ntimeout error\nerror\ntimeout\nabab\naba\nerror error retry\n\n'
    ref = AllTermsRef([text])
    ids = lambda g: ref.search_all_ids(g).tolist()
    assert ids([b'error']) == [0, 1, 2, 6]
    assert ids([b'error', b'timeout']) == ids([b'timeout', b'error']) == [0, 1]          # either order in the entry
    assert ids(([b'error'], [b'timeout'])) == [2, 6]
    assert ids(([b'error'], [b'retry'])) == [0, 1, 2]
    assert ids(([b'error', b'timeout'], [b'retry'])) == [0, 1]                            # an exclude that removes none
    assert ids(([b'error'], [b'r'])) == []                                                # ... all
    assert ids([b'error', b'error']) == [0, 1, 2, 6]                                      # a repeated term
    assert ids(([b'error'], [b'error'])) == []                                            # include == exclude
    assert ids([b'error error']) == [6] and ids([b'error', b'error error']) == [6]        # a term twice in an entry
    assert ids([b'aba', b'bab']) == [4]                                                   # overlapping terms in 'abab'
    assert ids([b'aba']) == [4, 5] and ids(([b'aba'], [b'bab'])) == [5]
    assert ids([b'timeout', b'timeout error']) == [1]                                     # a term equal to the whole entry
    assert ids([b'error', b'missing']) == [] and ids([b'missing']) == []
    # newlines: an include term with one empties the group, an exclude term with one excludes nothing -- although
    # bytes.find sees 'error\ntimeout' in the text
    assert text.find(b'error\ntimeout') >= 0
    assert ids([b'error', b'error\ntimeout']) == [] and ids([b'\n']) == []
    assert ids(([b'error'], [b'error\ntimeout'])) == [0, 1, 2, 6] and ids(([b'error'], [b'\n'])) == [0, 1, 2, 6]


def test_reference_on_chunk_edges_and_file_indexes():
    # chunk 4: entry at offset 0, an empty entry; chunk 7: no closing newline, 'ab' ends at the very last byte
    ref = AllTermsRef([b'ab x\n\nx ab\n', b'x\nab\nx ab'], indices=[4, 7])
    a, c = 4 << 32, 7 << 32
    assert ref.search_all_ids([b'ab']).tolist() == [a, a | 2, c | 1, c | 2]
    assert ref.search_all_ids([b'ab', b'x']).tolist() == [a, a | 2, c | 2]
    assert ref.search_all_ids(([b'x'], [b'ab'])).tolist() == [c]
    assert ref.search_all_ids([b'x ab', b'b']).tolist() == [a | 2, c | 2]          # the last byte of the unterminated entry counts
    assert ref.entry(c | 2) == b'x a'                                               # ... though the text handed out loses it
    assert ref.search_all_ids([b'b\x00']).tolist() == []
    assert ref.search_all_ids([b'ab', b'ab x']).tolist() == [a]                     # 'ab x' occurs in chunk 4 only
    assert AllTermsRef([b'']).search_all_ids([b'a']).size == 0


def test_reference_agrees_with_set_operations_over_the_lines():
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b'ab\n', np.uint8)
    terms = [b'a', b'b', b'ab', b'ba', b'aa', b'aba', b'bab', b'abab']
    for _ in range(40):
        n = int(rng.integers(1, 120))
        text = bytes(alphabet[rng.choice(3, n, p=[0.45, 0.35, 0.2])])[:-1] + b'\n'
        lines = text[:-1].split(b'\n')
        ref = AllTermsRef([text])
        for _ in range(12):
            k, x = int(rng.integers(1, 4)), int(rng.integers(0, 3))
            inc = [terms[int(i)] for i in rng.integers(0, len(terms), k)]
            exc = [terms[int(i)] for i in rng.integers(0, len(terms), x)]
            want = [i for i, ln in enumerate(lines) if all(t in ln for t in inc) and not any(t in ln for t in exc)]
            assert ref.search_all_ids((inc, exc)).tolist() == want, (text, inc, exc)
            if not exc:
                assert ref.search_all_ids(inc).tolist() == want


def test_split_group_takes_both_spellings():
    assert split_group([b'a', b'b']) == ([b'a', b'b'], [])
    assert split_group(([b'a'], [b'b'])) == ([b'a'], [b'b'])
    assert split_group(((b'a', b'c'), ())) == ([b'a', b'c'], [])
    assert split_group([b'a']) == ([b'a'], [])


# ---- the surface -----------------------------------------------------------------------------------------------------

def test_library_exports_and_binding_declares_the_entry_points():
    from pysubstringsearch_amd import _ffi
    raw = ctypes.CDLL(os.path.join(ROOT, 'pysubstringsearch_amd', 'libpss.so'))
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in SYMBOLS:
        assert hasattr(raw, name), f'{name} is not exported by libpss.so'
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int
    assert list(_ffi.lib.pss_reader_search_terms_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_terms_ids_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_terms_batch.argtypes) == [vp, vp, vp, u32, vp, u32, vp, vp]


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
        assert list(inspect.signature(getattr(P.Reader, name)).parameters) == ['self', 'groups']
    for name in METHODS[3:]:
        assert list(inspect.signature(getattr(P.Reader, name)).parameters) == ['self', 'terms', 'exclude']


def test_groups_are_packed_for_the_library():
    import pysubstringsearch_amd as P
    blob, offs, goff, excl = P.Reader._terms_args([[b'ab', b'c'], ([b'x'], [b'yz', b'ab']), ((b'q',), ())])
    assert blob == b'abcxyzabq' and offs.tolist() == [0, 2, 3, 4, 6, 8, 9]
    assert goff.tolist() == [0, 2, 5, 6] and goff.dtype == np.uint64
    assert excl.tolist() == [0, 0, 0, 1, 1, 0] and excl.dtype == np.uint8
    blob, offs, goff, excl = P.Reader._terms_args([])
    assert blob == b'' and offs.tolist() == [0] and goff.tolist() == [0]
    r = P.Reader._from_handle(ctypes.c_void_p())
    with pytest.raises(ValueError, match='closed Reader'):
        r.count_all_bytes([[b'a']])


@pytest.mark.parametrize('bad,what', [([[]], 'no include term'), ([([], [b'a'])], 'no include term'), ([[b'a'], ([], [])], 'no include term'),
                                      ([[b'a', b'']], 'empty term'), ([([b'a'], [b''])], 'empty term')])
def test_bad_groups_are_a_value_error_before_the_library_is_called(bad, what):
    import pysubstringsearch_amd as P
    r = P.Reader._from_handle(ctypes.c_void_p())      # (closed: reaching the library would raise 'closed Reader' instead)
    for call in (r.search_all_batch_packed, r.search_all_ids_batch, r.count_all_bytes):
        with pytest.raises(ValueError, match=what):
            call(bad)


def test_the_conveniences_take_str_only():
    import pysubstringsearch_amd as P
    r = P.Reader._from_handle(ctypes.c_void_p())
    for bad in (b'error', [b'error'], 'error'):
        with pytest.raises(TypeError):
            r.search_all(bad)
        with pytest.raises(TypeError):
            r.count_all(bad)
    with pytest.raises(TypeError):
        r.search_all(['error'], exclude=[b'retry'])
    with pytest.raises(TypeError):
        r.search_all_ids_batch([b'a bare byte string is not a group'])
    with pytest.raises(ValueError, match='no include term'):
        r.search_all([], exclude=['retry'])


def c_batch(terms, goff, excl):
    blob = b''.join(terms)
    offs = np.cumsum([0] + [len(t) for t in terms]).astype(np.uint64)
    return blob, offs, np.array(goff, dtype=np.uint64), np.array(excl if excl else [0], dtype=np.uint8)


BAD_C_BATCHES = [
    ('no include term', [b'a', b'b'], [0, 1, 2], [0, 1]),
    ('no include term', [b'a'], [0, 0, 1], [0]),                  # an empty group
    ('is empty', [b'a', b''], [0, 2], [0, 0]),
    ('exclude[1] = 2', [b'a', b'b'], [0, 2], [0, 2]),
    ('exclude[0] = 255', [b'a', b'b'], [0, 2], [255, 0]),
    ('group offsets', [b'a', b'b'], [1, 2], [0, 0]),              # does not start at 0
    ('group offsets', [b'a', b'b'], [0, 1], [0, 0]),              # does not end at nterms
    ('group offsets', [b'a', b'b', b'c'], [0, 2, 1, 3], [0, 0, 0]),      # decreases
    ('group offsets', [b'a', b'b'], [0, 3, 2], [0, 0]),           # passes nterms
]


@pytest.mark.parametrize('what,terms,goff,excl', BAD_C_BATCHES)
def test_bad_batches_are_refused_by_the_c_calls(what, terms, goff, excl):
    """PSS_EINVAL with a message, *out and counts untouched.  The batch is judged before the reader is, so no device is
    needed; tests/test_all_terms_gpu.py repeats the calls on a live reader."""
    from pysubstringsearch_amd import _ffi
    blob, offs, g, e = c_batch(terms, goff, excl)
    ng = len(goff) - 1
    for fn in (_ffi.lib.pss_reader_search_terms_batch, _ffi.lib.pss_reader_search_terms_ids_batch):
        out = ctypes.c_void_p()
        assert fn(None, blob, offs.ctypes.data, len(terms), g.ctypes.data, ng, e.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert not out.value and what in _ffi.last_error(), _ffi.last_error()
    counts = np.full(4, 7, dtype=np.uint64)
    assert _ffi.lib.pss_reader_count_terms_batch(None, blob, offs.ctypes.data, len(terms), g.ctypes.data, ng, e.ctypes.data,
                                                 counts.ctypes.data) == _ffi.PSS_EINVAL
    assert counts.tolist() == [7] * 4 and what in _ffi.last_error()


def test_null_arguments_are_refused_with_a_status():
    from pysubstringsearch_amd import _ffi
    blob, offs, g, e = c_batch([b'a', b'b'], [0, 2], [0, 1])
    out = ctypes.c_void_p()
    args = (blob, offs.ctypes.data, 2, g.ctypes.data, 1, e.ctypes.data)
    assert _ffi.lib.pss_reader_search_terms_batch(None, *args, ctypes.byref(out)) == _ffi.PSS_EINVAL       # a good batch, no reader
    assert 'pss_reader_search_terms_batch' in _ffi.last_error() and 'no reader' in _ffi.last_error()
    assert _ffi.lib.pss_reader_search_terms_ids_batch(None, *args, None) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_count_terms_batch(None, *args, None) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_terms_batch(None, blob, offs.ctypes.data, 2, None, 1, e.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_search_terms_batch(None, blob, offs.ctypes.data, 2, g.ctypes.data, 1, None, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert not out.value
