"""The host side of the any-of search (include/pss.h, the three pss_reader_*_any_* calls and pss_any_alternatives; DESIGN.md
4.22): no reader, no GPU.  The normalisation table; the caps and the other refusals of the Python layer and of the C layer, in
the documented order; any_alternatives against the reference's restatement (tests/any_ref.py); the request rule and the
block's layout against csrc/search_layout.h and csrc/any_terms.h on the CPU; the declarations."""
import ctypes
import inspect
import os
import pathlib
import subprocess

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi
from tests import any_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_CALLS = ('pss_reader_search_any_batch', 'pss_reader_search_any_ids_batch', 'pss_reader_count_any_batch')
BATCHED = ('search_any_batch_packed', 'search_any_ids_batch', 'count_any_bytes')
METHODS = BATCHED + ('search_any', 'count_any')


def alts_of(terms, icase=False, letters=None):
    return [a for a, _, _ in pss.any_alternatives(terms, icase, letters)]


# ---- the normalisation -----------------------------------------------------------------------------------------------------

TABLE = [
    # (what, the set, icase, what is left)
    ('duplicates', [b'warn', b'error', b'warn', b'warn'], False, [b'error', b'warn']),
    ('the sort, bytewise: upper case first', [b'warn', b'error', b'Fatal', b'\xff', b'~'], False, [b'Fatal', b'error', b'warn', b'~', b'\xff']),
    ('a prefix drops the longer one', [b'error', b'errors', b'err'], False, [b'err']),
    ('a substring anywhere drops the longer one', [b'xerrorx', b'error', b'terror'], False, [b'error']),
    ('overlapping alternatives both stay', [b'abc', b'bcd'], False, [b'abc', b'bcd']),
    ('a newline voids its alternative, not its set', [b'a\nb', b'cd', b'\n'], False, [b'cd']),
    ('a set voided by newlines', [b'a\nb', b'\n'], False, []),
    ('what holds a newline drops nothing', [b'ab\ncd', b'ab\ncdx', b'q'], False, [b'q']),
    ('exact bytes: the cases are different strings', [b'Warn', b'warn', b'WARN'], False, [b'WARN', b'Warn', b'warn']),
    ('the fold', [b'Warn', b'warn', b'WARN', b'ERROR'], True, [b'error', b'warn']),
    ('the fold makes substrings', [b'ERR', b'xerrx'], True, [b'err']),
    ('@ and ` stay distinct', [b'@', b'`'], True, [b'@', b'`']),
    ('[ and { stay distinct', [b'[', b'{'], True, [b'[', b'{']),
    ('0xC9 and 0xE9 stay distinct', [b'\xc9', b'\xe9'], True, [b'\xc9', b'\xe9']),
    ('0x00 is a byte like any other', [b'a\x00', b'a\x00b', b'\x00c'], False, [b'\x00c', b'a\x00']),
]


@pytest.mark.parametrize('what,given,icase,left', TABLE, ids=[t[0] for t in TABLE])
def test_normalisation_table(what, given, icase, left):
    assert alts_of(given, icase) == left, what
    assert any_ref.normalise(given, icase) == left, what
    # prefix-free, and as strong as the set it came from: an entry holds one of `given` iff it holds one of `left`
    assert not any(a != b and b.startswith(a) for a in left for b in left)
    assert not left or alts_of(left, icase) == left      # idempotent (an empty set is refused, and none is ever asked for)
    assert alts_of(list(reversed(given)), icase) == left


def test_any_alternatives_restates_the_seed_rule():
    """Exact: every alternative is its own query at 0.  Under fold: the seed of every alternative under the set's F =
    min(letters, floor(log2(64 / alternatives))), against a search over every window."""
    rng = np.random.default_rng(2200)
    alphabet = np.frombuffer(b'aAbBcz1@`\xe9\x00\n', np.uint8)
    sets = [[b'error', b'WARN', b'fatal'], [b'ab1234', b'cb1234'], [b'Password'], [b'12345678'], [b'a'], [b'1a2b3c4d5e6f7g8h', b'@`[{']]
    sets += [[bytes(alphabet[rng.integers(0, len(alphabet), int(rng.integers(1, 14)))]) for _ in range(int(rng.integers(1, 40)))]
             for _ in range(60)]
    folded = shared = 0
    for given in sets:
        exact = pss.any_alternatives(given)
        assert exact == any_ref.alternatives(given) and all(pos == 0 and seed == a for a, pos, seed in exact)
        for letters in (None, 1, 2, 3, 4, 5, 6):
            if len(any_ref.normalise(given, True)) > any_ref.MAX_ALTS_ICASE:
                with pytest.raises(ValueError, match='after normalisation'):
                    pss.any_alternatives(given, True, letters)
                continue
            got = pss.any_alternatives(given, True, letters)
            want = any_ref.alternatives(given, True, any_ref.LETTERS if letters is None else letters)
            assert got == want, (given, letters)
            f = any_ref.seed_letters(len(got), any_ref.LETTERS if letters is None else letters) if got else 0
            for a, pos, seed in got:
                assert a[pos:pos + len(seed)] == seed and sum(any_ref.is_letter(b) for b in seed) <= f and a == a.lower()
            assert sum(len(any_ref.spellings(seed)) for _, _, seed in got) <= 64
            folded += bool(got)
            shared += len({seed for _, _, seed in got}) < len(got)
    assert folded > 200 and shared > 5
    assert pss.any_alternatives([b'ab1234', b'cb1234'], True, 1) == [(b'ab1234', 1, b'b1234'), (b'cb1234', 1, b'b1234')]
    assert any_ref.seed_letters(1) == 5 and any_ref.seed_letters(1, 6) == 6 and [any_ref.seed_letters(n, 6) for n in (2, 3, 4, 5, 8, 9, 16, 17, 32)] == \
        [5, 4, 4, 3, 3, 2, 2, 1, 1]


def test_the_configured_letters(monkeypatch):
    given = [b'abcdefgh']
    try:
        for F in (1, 3, 6):
            monkeypatch.setenv('PSS_ICASE_SEED_LETTERS', str(F))
            _ffi.lib.pss_reload_env()
            assert pss.any_alternatives(given, True) == any_ref.alternatives(given, True, F) == [(b'abcdefgh', 0, b'abcdefgh'[:F])]
            assert pss.any_alternatives(given, True, 2) == [(b'abcdefgh', 0, b'ab')]
    finally:
        monkeypatch.delenv('PSS_ICASE_SEED_LETTERS', raising=False)
        _ffi.lib.pss_reload_env()


# ---- the refusals ------------------------------------------------------------------------------------------------------------

def distinct(n):
    """n alternatives none of which holds another: two bytes each, all different."""
    return [bytes([0x30 + i // 10, 0x61 + i % 10]) for i in range(n)]


def test_the_caps_sit_at_64_and_32():
    assert len(alts_of(distinct(64))) == 64
    with pytest.raises(ValueError, match='65 alternatives after normalisation, more than the 64'):
        pss.any_alternatives(distinct(65))
    assert len(alts_of(distinct(32), True)) == 32
    with pytest.raises(ValueError, match='33 alternatives after normalisation, more than the 32'):
        pss.any_alternatives(distinct(33), True)
    # the cap is judged AFTER normalisation: duplicates, newlines and superstrings do not count
    many = distinct(64) + distinct(64) + [a + b'\n' for a in distinct(40)] + [b'x' + a + b'y' for a in distinct(30)]
    assert len(alts_of(many)) == 64
    assert len(alts_of([a.upper() for a in distinct(32)] + distinct(32), True)) == 32
    # under fold a full set still has a seed of one letter per alternative: 64 queries
    assert all(sum(any_ref.is_letter(b) for b in seed) == 1 for _, _, seed in pss.any_alternatives(distinct(32), True))


def test_python_refusals_need_no_reader():
    r = object.__new__(pss.Reader)
    for name in BATCHED:
        call = getattr(r, name)
        with pytest.raises(ValueError, match='set 1: no alternative'):
            call([[b'a'], []])
        with pytest.raises(ValueError, match='set 0: an empty alternative'):
            call([[b'a', b'']])
        with pytest.raises(TypeError, match='set 1: an alternative must be bytes, not str'):
            call([[b'a'], [b'b', 'c']])
        for bare in (b'abc', 'abc', bytearray(b'abc')):
            with pytest.raises(TypeError, match='cannot be converted to a sequence of sets'):
                call(bare)
            with pytest.raises(TypeError, match='set 0: .* cannot be converted to a sequence of alternatives'):
                call([bare])
        for bad in (1, 0, None, 'yes', [True], np.bool_(True)):
            with pytest.raises(TypeError, match="argument 'icase'"):
                call([[b'a']], icase=bad)
        with pytest.raises(TypeError):                   # keyword only
            call([[b'a']], True)
    for name in ('search_any', 'count_any'):
        call = getattr(r, name)
        for bare in ('error', b'error'):
            with pytest.raises(TypeError, match="argument 'terms'"):
                call(bare)
        with pytest.raises(TypeError, match='PyString'):
            call([b'error'])
        with pytest.raises(ValueError, match='no alternative'):
            call([])
        with pytest.raises(ValueError, match='an empty alternative'):
            call(['a', ''])
        with pytest.raises(TypeError, match="argument 'icase'"):
            call(['a'], icase=1)
        with pytest.raises(TypeError):
            call(['a'], True)


def test_any_alternatives_argument_checks():
    with pytest.raises(TypeError, match='sequence of alternatives'):
        pss.any_alternatives(b'abc')
    with pytest.raises(TypeError, match='sequence of alternatives'):
        pss.any_alternatives('abc')
    with pytest.raises(TypeError, match='must be bytes'):
        pss.any_alternatives(['abc'])
    with pytest.raises(TypeError, match="argument 'icase'"):
        pss.any_alternatives([b'abc'], 1)
    with pytest.raises(ValueError, match='no alternative'):
        pss.any_alternatives([])
    with pytest.raises(ValueError, match='empty alternative'):
        pss.any_alternatives([b'a', b''])
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match='1 .. 6'):
            pss.any_alternatives([b'abc'], True, bad)
    assert pss.any_alternatives([b'a\n']) == [] and pss.any_alternatives([b'A\n', b'\n'], True) == []


# ---- the C layer, without a reader -------------------------------------------------------------------------------------------

def c_sets(sets, aoffsets=None, set_offsets=None):
    alts = [a for s in sets for a in s]
    blob = b''.join(alts) or b'\x00'
    aoff = np.cumsum([0] + [len(a) for a in alts]).astype(np.uint64) if aoffsets is None else np.array(aoffsets, dtype=np.uint64)
    soff = np.cumsum([0] + [len(s) for s in sets]).astype(np.uint64) if set_offsets is None else np.array(set_offsets, dtype=np.uint64)
    return blob, aoff, len(alts), soff, len(sets)


def test_einval_order_with_a_null_reader():
    """Null out, null bytes or offsets with a count above 0, unknown flags, bad offsets, the first bad set as "set <g>: ...",
    and the null reader last: each refusal comes with everything AFTER it in that order wrong as well."""
    lib = _ffi.lib
    searches = (lib.pss_reader_search_any_batch, lib.pss_reader_search_any_ids_batch)

    def refused(what, blob, aoff, nalts, soff, nsets, flags=0, out_ok=True):
        aoff_p = None if aoff is None else aoff.ctypes.data
        soff_p = None if soff is None else soff.ctypes.data
        for fn in searches:
            out = ctypes.c_void_p()
            assert fn(None, blob, aoff_p, nalts, soff_p, nsets, flags, ctypes.byref(out) if out_ok else None) == _ffi.PSS_EINVAL
            assert not out.value and fn.__name__ in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())
        counts = np.full(4, 7, dtype=np.uint64)
        assert lib.pss_reader_count_any_batch(None, blob, aoff_p, nalts, soff_p, nsets, flags, counts.ctypes.data if out_ok else None) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pss_reader_count_any_batch' in _ffi.last_error() and what in _ffi.last_error(), \
            (what, _ffi.last_error())

    good = c_sets([[b'ab', b'c'], [b'd']])
    blob, aoff, nalts, soff, nsets = good
    bad_set = c_sets([[b'ab'], [b'c', b'']])
    bad_aoff = np.array([1, 2, 3, 4], dtype=np.uint64)
    # 1. the output argument, whatever else is wrong
    refused('bad arguments', None, None, nalts, None, nsets, flags=6, out_ok=False)
    # 2. null bytes / offsets with a count above 0, whatever flags, offsets and sets say
    refused('bad arguments', None, bad_aoff, nalts, soff, nsets, flags=6)
    refused('bad arguments', blob, None, nalts, soff, nsets, flags=6)
    refused('bad arguments', blob, bad_aoff, nalts, None, nsets, flags=6)
    # 3. unknown flags, whatever offsets and sets say
    refused('flags = 6', blob, bad_aoff, nalts, soff, nsets, flags=6)
    refused('flags = 2', *bad_set, flags=2)
    # 4. bad offsets, whatever the sets say
    refused('the alternative offsets start at 1, not at 0', blob, bad_aoff, nalts, soff, nsets)
    refused('the alternative offsets decrease at alternative 1', *c_sets([[b'abc', b'c'], []], aoffsets=[0, 3, 2]))
    refused('the set offsets start at 1, not at 0', *c_sets([[b'ab', b'c'], []], set_offsets=[1, 2, 2]))
    refused('the set offsets decrease at set 1', *c_sets([[b'ab', b''], [b'd']], set_offsets=[0, 2, 1]))
    refused('the set offsets end at 2, not at the 3 alternatives', *c_sets([[b'ab', b''], [b'd']], set_offsets=[0, 1, 2]))
    # 5. the first bad set, by its number, under either flag
    for flags in (0, _ffi.ANY_ICASE):
        refused('set 1: alternative 1 is empty', *bad_set, flags=flags)
        refused('set 1: no alternative', *c_sets([[b'a'], [], [b'']]), flags=flags)
        refused('set 2: no alternative', *c_sets([[b'a'], [b'b\n'], []]), flags=flags)
    refused('set 1: 65 alternatives after normalisation, more than the 64', *c_sets([distinct(64), distinct(65), []]))
    refused('set 0: 33 alternatives after normalisation, more than the 32 a set takes under PSS_ANY_ICASE',
            *c_sets([distinct(33), distinct(65)]), flags=_ffi.ANY_ICASE)
    # 6. the null reader, last: every well-formed batch gets this far
    refused('no reader', *good)
    refused('no reader', *good, flags=_ffi.ANY_ICASE)
    refused('no reader', *c_sets([distinct(64), distinct(64) + [b'zz\n']]))
    refused('no reader', *c_sets([distinct(32), [b'\n']]), flags=_ffi.ANY_ICASE)
    refused('no reader', *c_sets([]))
    refused('no reader', b'\x00', None, 0, None, 0)


def test_pss_any_alternatives_in_c():
    lib = _ffi.lib
    blob, aoff, nalts, _, _ = c_sets([[b'Warn', b'error', b'ERRORS', b'x\n']])
    out = ctypes.create_string_buffer(64)
    ooff, pos, ln, cnt = np.zeros(nalts + 1, np.uint64), np.zeros(nalts, np.uint32), np.zeros(nalts, np.uint32), ctypes.c_uint32(99)

    def call(flags=0, letters=0, cap=64, out_=out, cnt_=cnt):
        return lib.pss_any_alternatives(blob, aoff.ctypes.data, nalts, flags, letters, out_, cap, ooff.ctypes.data, pos.ctypes.data,
                                        ln.ctypes.data, ctypes.byref(cnt_) if cnt_ is not None else None)

    assert call() == _ffi.PSS_OK and cnt.value == 3 and ooff[:4].tolist() == [0, 6, 10, 15] and out.raw[:15] == b'ERRORSWarnerror'
    assert pos[:3].tolist() == [0, 0, 0] and ln[:3].tolist() == [6, 4, 5]
    assert call(_ffi.ANY_ICASE, 2) == _ffi.PSS_OK and cnt.value == 2 and out.raw[:9] == b'errorwarn' and ln[:2].tolist() == [2, 2]
    assert call(cap=14) == _ffi.PSS_EINVAL and 'need 15 bytes' in _ffi.last_error()
    assert call(letters=7) == _ffi.PSS_EINVAL and 'letters = 7' in _ffi.last_error()
    assert call(out_=None) == _ffi.PSS_EINVAL and call(cnt_=None) == _ffi.PSS_EINVAL
    assert call(flags=4) == _ffi.PSS_EINVAL and 'flags = 4' in _ffi.last_error()


# ---- the request rule and the layout -------------------------------------------------------------------------------------------

def test_the_request_rule_on_the_cpu(tmp_path):
    """tests/native/any_request.cpp against csrc/search_layout.h and csrc/any_terms.h alone, under AddressSanitizer + UBSan:
    one valid request in exact bytes and one under fold, every clause of any_request_ok broken in turn, the block's layout
    held to a restated table, the normalisation on a few sets."""
    csrc = os.path.join(ROOT, 'pysubstringsearch_amd', 'csrc')
    exe = str(tmp_path / 'any_request')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I' + csrc,
                        os.path.join(ROOT, 'tests', 'native', 'any_request.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'any_request: ok' in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_declarations():
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    for name in C_CALLS + ('pss_any_alternatives',):
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    assert list(_ffi.lib.pss_reader_search_any_batch.argtypes) == [vp, vp, vp, u32, vp, u32, u32, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_any_ids_batch.argtypes) == [vp, vp, vp, u32, vp, u32, u32, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_any_batch.argtypes) == [vp, vp, vp, u32, vp, u32, u32, vp]
    assert list(_ffi.lib.pss_any_alternatives.argtypes) == [vp, vp, u32, u32, i32, vp, u64, vp, vp, vp, ctypes.POINTER(u32)]
    assert '#define PSS_ANY_ICASE 1u' in hdr and _ffi.ANY_ICASE == 1
    assert '#define PSS_ANY_MAX_ALTS 64u' in hdr and '#define PSS_ANY_MAX_ALTS_ICASE 32u' in hdr
    assert (_ffi.ANY_MAX_ALTS, _ffi.ANY_MAX_ALTS_ICASE) == (any_ref.MAX_ALTS, any_ref.MAX_ALTS_ICASE) == (64, 32)
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    assert 'def any_alternatives(terms: typing.Sequence[bytes], icase: bool = False, letters: typing.Optional[int] = None)' in stub
    assert 'any_alternatives' in pss.__all__
    for name in METHODS:
        assert '*, icase: bool = False' in next(ln for ln in stub.splitlines() if f'def {name}(' in ln), name
        par = inspect.signature(getattr(pss.Reader, name)).parameters['icase']
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY, name
    # no route bit and no environment switch of its own
    assert not any('ANY' in name for name in _ffi.ROUTES) and 'PSS_NO_ANY' not in hdr
