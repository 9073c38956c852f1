"""The host side of the case-insensitive search (include/pss.h, pss_icase_variants and the argument checks of the three
pss_reader_*_icase_* calls): no reader, no GPU.  The seed is the pattern's longest window with at most F ASCII letters,
the leftmost on a tie; its 2^f spellings come in ascending byte order."""
import ctypes
import itertools

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi, icase_variants

ALPHABET = b'aZ@[`{1_\x80\xc1\xe1\x00'
LETTERS = range(1, 7)


def is_letter(b: int) -> bool:
    return 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A


def seed_window(p: bytes, F: int):
    """(offset, length) of the longest window of p with at most F ASCII letters, the leftmost on a tie."""
    best = (0, 0)
    for i in range(len(p)):
        k, j = 0, i
        while j < len(p) and k + is_letter(p[j]) <= F:
            k += is_letter(p[j])
            j += 1
        if j - i > best[1]:
            best = (i, j - i)
    return best


def all_spellings(seed: bytes):
    choices = [(bytes([b & ~0x20]), bytes([b | 0x20])) if is_letter(b) else (bytes([b]),) for b in seed]
    return {b''.join(c) for c in itertools.product(*choices)}


def random_patterns():
    rng = np.random.default_rng(1301)
    abc = np.frombuffer(ALPHABET, np.uint8)
    out = [bytes(abc[rng.integers(0, len(abc), int(rng.integers(1, 24)))]) for _ in range(300)]
    return out + [b'Error', b'user_id=12345678', b'abcdefgh', b'a', b'Z', b'aZaZaZaZaZaZ', b'ab12cd34ef56gh', b'1a2', b'aaaaaaa1bbbbbbb']


@pytest.mark.parametrize('F', LETTERS)
def test_variants_are_all_spellings_of_the_seed_ascending(F):
    for p in random_patterns():
        off, var = icase_variants(p, F)
        want_off, want_len = seed_window(p, F)
        assert (off, len(var[0])) == (want_off, want_len), (p, F)
        seed = p[off:off + want_len]
        f = sum(is_letter(b) for b in seed)
        assert f <= F and len(var) == 2 ** f, (p, F)
        assert all(a < b for a, b in zip(var, var[1:])), (p, F)                 # strictly ascending bytewise
        assert all(v.lower() == seed.lower() and len(v) == len(seed) for v in var)
        assert set(var) == all_spellings(seed)
        # only A .. Z / a .. z vary: every other byte is the pattern's own
        assert all(v[i] == seed[i] for v in var for i in range(len(seed)) if not is_letter(seed[i]))


def test_seed_examples():
    assert icase_variants(b'user_id=12345678', 5)[0] == 1 and icase_variants(b'user_id=12345678', 5)[1][-1] == b'ser_id=12345678'
    assert icase_variants(b'Error', 2) == (0, [b'ER', b'Er', b'eR', b'er'])
    assert icase_variants(b'abcdefgh', 6)[1][0] == b'ABCDEF' and icase_variants(b'abcdefgh', 2) == (0, [b'AB', b'Ab', b'aB', b'ab'])
    assert icase_variants(b'12ab', 1) == (0, [b'12A', b'12a'])                  # the leftmost of two windows of three bytes
    assert icase_variants(b'ab__c', 1) == (1, [b'B__', b'b__'])                 # 'b__' and '__c' tie: the leftmost
    assert icase_variants(b'@[`{\xc1\xe1', 1) == (0, [b'@[`{\xc1\xe1'])         # bytes beside the letters do not fold


def test_letterless_pattern_is_its_own_only_variant():
    for p in (b'1', b'12345', b'@[`{', b'\x00\x20', b'\xc1\xe1\x80\xff', b'1\n2', b'_' * 300):
        for F in LETTERS:
            assert icase_variants(p, F) == (0, [p])
        assert icase_variants(p) == (0, [p])


def test_configured_letters_and_the_knob(monkeypatch):
    names = {}
    for i in range(_ffi.lib.pss_knob_count()):
        name, dflt, fuzz, what = (ctypes.c_char_p() for _ in range(4))
        _ffi.check(_ffi.lib.pss_knob_info(i, ctypes.byref(name), ctypes.byref(dflt), ctypes.byref(fuzz), ctypes.byref(what)))
        names[name.value.decode()] = (dflt.value.decode(), fuzz.value.decode())
    assert names['PSS_ICASE_SEED_LETTERS'] == ('5', '1|2|3|4|5|6')
    monkeypatch.delenv('PSS_ICASE_SEED_LETTERS', raising=False)
    _ffi.check(_ffi.lib.pss_reload_env())
    assert icase_variants(b'abcdefgh') == icase_variants(b'abcdefgh', 5) and len(icase_variants(b'abcdefgh')[1]) == 32
    try:
        for F in LETTERS:
            monkeypatch.setenv('PSS_ICASE_SEED_LETTERS', str(F))
            _ffi.check(_ffi.lib.pss_reload_env())
            assert icase_variants(b'abcdefgh') == icase_variants(b'abcdefgh', F)
            assert icase_variants(b'abcdefgh', 3) == (0, [b'ABC', b'ABc', b'AbC', b'Abc', b'aBC', b'aBc', b'abC', b'abc'])
    finally:
        monkeypatch.delenv('PSS_ICASE_SEED_LETTERS', raising=False)
        _ffi.check(_ffi.lib.pss_reload_env())


def test_variants_errors():
    with pytest.raises(ValueError, match='empty'):
        icase_variants(b'')
    for bad in (0, 7, -1, 64):
        with pytest.raises(ValueError):
            icase_variants(b'abc', bad)
    for bad in ('abc', None, 5):
        with pytest.raises(TypeError):
            icase_variants(bad)
    off, ln, cnt = ctypes.c_uint32(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    args = (ctypes.byref(off), ctypes.byref(ln), ctypes.byref(cnt))
    lib = _ffi.lib
    assert lib.pss_icase_variants(b'', 0, 0, None, 0, *args) == _ffi.PSS_EINVAL and 'empty' in _ffi.last_error()
    assert lib.pss_icase_variants(None, 3, 0, None, 0, *args) == _ffi.PSS_EINVAL
    assert lib.pss_icase_variants(b'abc', 3, 7, None, 0, *args) == _ffi.PSS_EINVAL and 'letters = 7' in _ffi.last_error()
    assert lib.pss_icase_variants(b'abc', 3, 2, None, 0, None, ctypes.byref(ln), ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert (off.value, ln.value, cnt.value) == (7, 7, 7)
    buf = ctypes.create_string_buffer(8)
    assert lib.pss_icase_variants(b'abc', 3, 2, buf, 7, *args) == _ffi.PSS_EINVAL and 'need more' in _ffi.last_error()
    assert lib.pss_icase_variants(b'abc', 3, 2, buf, 8, *args) == _ffi.PSS_OK
    assert (off.value, ln.value, cnt.value) == (0, 2, 4) and buf.raw == b'ABAbaBab'


def c_batch(patterns, offsets=None):
    blob = b''.join(patterns)
    offs = np.cumsum([0] + [len(t) for t in patterns]).astype(np.uint64) if offsets is None else np.array(offsets, dtype=np.uint64)
    return blob, offs


def test_einval_cases_with_a_null_reader():
    """Every malformed batch is reported as such without a reader; the null reader is judged last."""
    lib = _ffi.lib
    searches = (lib.pss_reader_search_icase_batch, lib.pss_reader_search_icase_ids_batch)

    def refused(what, blob, offs, nq, out_ok=True):
        offs_p = None if offs is None else offs.ctypes.data
        for fn in searches:
            out = ctypes.c_void_p()
            assert fn(None, blob, offs_p, nq, ctypes.byref(out) if out_ok else None) == _ffi.PSS_EINVAL
            assert not out.value and fn.__name__ in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())
        counts = np.full(4, 7, dtype=np.uint64)
        assert lib.pss_reader_count_icase_batch(None, blob, offs_p, nq, counts.ctypes.data if out_ok else None) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pss_reader_count_icase_batch' in _ffi.last_error() and what in _ffi.last_error()

    blob, offs = c_batch([b'ab', b'', b'c'])
    refused('pattern 1 is empty', blob, offs, 3)
    blob, offs = c_batch([b''])
    refused('pattern 0 is empty', blob, offs, 1)
    refused('start at 1, not at 0', *c_batch([b'ab', b'c'], [1, 2, 3]), 2)
    refused('decrease at pattern 1', *c_batch([b'abc', b'c'], [0, 3, 2]), 2)
    blob, offs = c_batch([b'ab', b'c'])
    refused('bad arguments', None, offs, 2)
    refused('bad arguments', blob, None, 2)
    refused('bad arguments', blob, offs, 2, out_ok=False)
    # a well-formed batch: the missing reader is what is left to report
    refused('no reader', blob, offs, 2)
    refused('no reader', *c_batch([b'Error\n', b'12', b'abcdefghijklmnopqrstuvwxyz' * 8]), 3)
    refused('no reader', b'', np.zeros(1, dtype=np.uint64), 0)


def test_the_expansion_must_fit_the_term_count_of_an_all_terms_batch(monkeypatch):
    """2^26 + 1 patterns of six letters expand to more than 2^32 - 1 spellings at F = 6.  No smaller batch can: a pattern
    has at most 64 spellings.  The batch itself costs the test 0.4 GB of pattern bytes and 0.5 GB of offsets; the library
    counts the terms in a pass of its own (one fold_seed per pattern, about a second) and refuses before it allocates
    anything."""
    nq = (1 << 26) + 1
    blob = np.tile(np.frombuffer(b'abcdef', np.uint8), nq)
    offs = np.arange(nq + 1, dtype=np.uint64) * np.uint64(6)
    monkeypatch.setenv('PSS_ICASE_SEED_LETTERS', '6')
    try:
        _ffi.check(_ffi.lib.pss_reload_env())
        out = ctypes.c_void_p()
        rc = _ffi.lib.pss_reader_search_icase_ids_batch(None, blob.ctypes.data, offs.ctypes.data, nq, ctypes.byref(out))
        assert rc == _ffi.PSS_EINVAL and not out.value and '2^32 - 1 terms' in _ffi.last_error()
    finally:
        monkeypatch.undo()
        _ffi.check(_ffi.lib.pss_reload_env())


def test_python_surface():
    assert 'icase_variants' in pss.__all__
    for name in ('search_icase_batch_packed', 'search_icase_ids_batch', 'count_icase_bytes', 'search_icase', 'count_icase'):
        doc = getattr(pss.Reader, name).__doc__
        assert doc and 'ASCII' in doc, name
