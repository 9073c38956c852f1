"""The surface of the anchored search without a GPU: the three C entry points are exported and bound, the route bit is
named, the Reader has the methods and the stubs name them, bad arguments are refused before any device is touched --
and the brute-force reference of tests/anchored_ref.py agrees with bytes.startswith / endswith / == over the lines of
random texts (tests/test_anchored_gpu.py runs the engine against it)."""
import ctypes
import os
import pathlib

import numpy as np
import pytest

from tests.anchored_ref import END, ENTRY, START, AnchoredRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pss_reader_search_anchored_batch', 'pss_reader_search_anchored_ids_batch', 'pss_reader_count_anchored_batch')
METHODS = ('search_anchored_batch_packed', 'search_anchored_ids_batch', 'count_anchored_bytes', 'search_prefix', 'search_suffix',
           'search_exact', 'has_entries')


def test_library_exports_and_binding_declares_the_entry_points():
    from pysubstringsearch_amd import _ffi
    raw = ctypes.CDLL(os.path.join(ROOT, 'pysubstringsearch_amd', 'libpss.so'))
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name in SYMBOLS:
        assert hasattr(raw, name), f'{name} is not exported by libpss.so'
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    assert list(_ffi.lib.pss_reader_search_anchored_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_anchored_ids_batch.argtypes) == [vp, vp, vp, u32, vp, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_anchored_batch.argtypes) == [vp, vp, vp, u32, vp, vp]
    assert '#define PSS_ANCHOR_START 1u' in hdr and '#define PSS_ANCHOR_END   2u' in hdr
    assert _ffi.ANCHORS == {'start': 1, 'end': 2, 'entry': 3}


def test_the_route_bit_is_named_on_both_sides():
    from pysubstringsearch_amd import _ffi
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    assert _ffi.ROUTES['ANCHORED'] == 0x2000
    assert '#define PSS_ROUTE_ANCHORED        0x2000u' in hdr
    assert len(set(_ffi.ROUTES.values())) == len(_ffi.ROUTES)
    # no struct changed size for it
    assert _ffi.lib.pss_search_stats_size() == ctypes.sizeof(_ffi.SearchStats) == 64


def test_reader_has_the_methods_and_the_stubs_name_them():
    import inspect

    import pysubstringsearch_amd as P
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in METHODS:
        assert hasattr(P.Reader, name), name
        assert f'def {name}(' in stub, f'{name} is missing from __init__.pyi'
    for name in METHODS[:3]:
        assert list(inspect.signature(getattr(P.Reader, name)).parameters) == ['self', 'patterns', 'anchors']
    # the reference's two calls keep their signatures
    assert list(inspect.signature(P.Reader.search).parameters) == ['self', 'substring']
    assert list(inspect.signature(P.Reader.search_multiple).parameters) == ['self', 'substrings']


def test_null_arguments_are_refused_with_a_status():
    from pysubstringsearch_amd import _ffi
    out = ctypes.c_void_p()
    anc = (ctypes.c_uint8 * 1)(1)
    offs = (ctypes.c_uint64 * 2)(0, 1)
    assert _ffi.lib.pss_reader_search_anchored_batch(None, b'a', offs, 1, anc, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert 'pss_reader_search_anchored_batch' in _ffi.last_error()
    assert _ffi.lib.pss_reader_search_anchored_ids_batch(None, b'a', offs, 1, anc, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_count_anchored_batch(None, b'a', offs, 1, anc, None) == _ffi.PSS_EINVAL
    assert not out.value


@pytest.mark.parametrize('bad', [0, 4, 3, 'START', 'prefix', '', None, b'start', ['start'], ['start', 'end', 'entry'], ['start', 1],
                                 ['start', 'exact'], [1, 2]])
def test_anchors_are_validated_in_python(bad):
    """Anything but 'start' | 'end' | 'entry', or one of them per pattern, is a ValueError before the library is called
    (the closed reader below would raise 'I/O operation on closed Reader' otherwise -- also a ValueError, hence the match)."""
    import pysubstringsearch_amd as P
    r = P.Reader._from_handle(ctypes.c_void_p())
    for call in (r.search_anchored_batch_packed, r.search_anchored_ids_batch, r.count_anchored_bytes):
        with pytest.raises(ValueError, match='anchor'):
            call([b'a', b'b'], bad)


def test_good_anchors_reach_the_library():
    import pysubstringsearch_amd as P
    blob, offs, anc = P.Reader._anchored_args([b'ab', b'', b'c'], ['start', 'entry', 'end'])
    assert blob == b'abc' and offs.tolist() == [0, 2, 2, 3] and anc.tolist() == [1, 3, 2] and anc.dtype == np.uint8
    assert P.Reader._anchored_args([b'x'] * 3, 'end')[2].tolist() == [2, 2, 2]
    assert P.Reader._anchored_args([], 'entry')[2].size == 0
    r = P.Reader._from_handle(ctypes.c_void_p())
    with pytest.raises(ValueError, match='closed Reader'):
        r.count_anchored_bytes([b'a'], 'start')


def test_reference_agrees_with_startswith_endswith_and_equality():
    """Texts with a closing newline: the entries are text[:-1].split(b'\\n'), so the three conditions are the three
    methods of bytes."""
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b'ab\n', np.uint8)
    for _ in range(60):
        n = int(rng.integers(1, 80))
        text = bytes(alphabet[rng.choice(3, n, p=[0.4, 0.3, 0.3])])[:-1] + b'\n'
        lines = text[:-1].split(b'\n')
        ref = AnchoredRef([text])
        assert ref.num_entries() == len(lines)
        pats = [b'', b'a', b'b', b'ab', b'ba', b'aa', b'aba', b'\n', b'a\n', b'\na', b'a\nb'] + [ln for ln in lines[:6]]
        for pat in pats:
            assert ref.search_ids(pat, START).tolist() == [i for i, ln in enumerate(lines) if ln.startswith(pat)], (text, pat)
            assert ref.search_ids(pat, END).tolist() == [i for i, ln in enumerate(lines) if ln.endswith(pat)], (text, pat)
            assert ref.search_ids(pat, ENTRY).tolist() == [i for i, ln in enumerate(lines) if ln == pat], (text, pat)
            assert ref.search_ids(pat, 'entry').tolist() == ref.search_ids(pat, ENTRY).tolist()
        for i, ln in enumerate(lines):
            assert ref.entry(i) == ln


def test_reference_on_a_text_without_a_closing_newline():
    """The unterminated last entry matches by its full text (the chunk text defines the match) and is handed out
    without its last byte (the engine's entry rule); ids carry the chunk's index in the file."""
    ref = AnchoredRef([b'ab\nxab\n', b'ab\n\nabab'], indices=[4, 7])
    assert ref.num_entries() == 2 + 3
    c = 7 << 32
    assert ref.search_ids(b'ab', START).tolist() == [4 << 32, c, c | 2]
    assert ref.search_ids(b'ab', END).tolist() == [4 << 32, (4 << 32) | 1, c, c | 2]
    assert ref.search_ids(b'abab', ENTRY).tolist() == [c | 2]
    assert ref.search_ids(b'aba', ENTRY).tolist() == []
    assert ref.search_ids(b'', ENTRY).tolist() == [c | 1]
    assert ref.search_ids(b'', START).size == ref.search_ids(b'', END).size == 5
    assert ref.entry(c | 2) == b'aba' and ref.entry(c | 1) == b'' and ref.entry((4 << 32) | 1) == b'xab'
    assert AnchoredRef([b'']).num_entries() == 0 and AnchoredRef([b'']).search_ids(b'', START).size == 0
    assert AnchoredRef([b'\n']).search_ids(b'', ENTRY).tolist() == [0]
