"""The surface of the entry ids without a GPU: the three C entry points are exported and bound, the Reader has the
methods, the stubs name them, and the calls refuse bad arguments with a status (tests/test_entry_ids_gpu.py runs them)."""
import ctypes
import os
import pathlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pss_reader_search_ids_batch', 'pss_reader_entries_by_id', 'pss_reader_chunk_entries')
METHODS = ('search_ids', 'search_ids_batch', 'entries_by_id', 'entries_by_id_packed', 'entry_counts', 'entry_ordinals')


def test_library_exports_and_binding_declares_the_entry_points():
    from pysubstringsearch_amd import _ffi
    raw = ctypes.CDLL(os.path.join(ROOT, 'pysubstringsearch_amd', 'libpss.so'))
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    for name in SYMBOLS:
        assert hasattr(raw, name), f'{name} is not exported by libpss.so'
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    assert list(_ffi.lib.pss_reader_search_ids_batch.argtypes) == [vp, vp, vp, u32, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_entries_by_id.argtypes) == [vp, vp, u64, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_chunk_entries.argtypes) == [vp, vp, vp, u64, ctypes.POINTER(u64)]


def test_reader_has_the_methods_and_the_stubs_name_them():
    import pysubstringsearch_amd as P
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    for name in METHODS:
        assert hasattr(P.Reader, name), name
        assert f'def {name}(' in stub, f'{name} is missing from __init__.pyi'
    assert isinstance(P.Reader.entry_counts, property)
    assert P.IdResult._fields == ('ids', 'counts') and 'IdResult' in P.__all__ and 'class IdResult' in stub


def test_null_arguments_are_refused_with_a_status():
    from pysubstringsearch_amd import _ffi
    out = ctypes.c_void_p()
    num = ctypes.c_uint64()
    assert _ffi.lib.pss_reader_search_ids_batch(None, None, None, 0, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_entries_by_id(None, None, 0, ctypes.byref(out)) == _ffi.PSS_EINVAL
    assert _ffi.lib.pss_reader_chunk_entries(None, None, None, 0, ctypes.byref(num)) == _ffi.PSS_EINVAL
    assert not out.value


def test_the_line_block_switch_is_registered():
    from pysubstringsearch_amd import _ffi
    knob = [k for k in _ffi.knobs() if k['name'] == 'PSS_LINE_BLOCK_SHIFT']
    assert len(knob) == 1 and knob[0]['default'] == '8'
