"""The host side of the match spans (include/pss.h, pss_reader_match_spans): no reader, no GPU.  The
argument contract of the C call without a reader and of the Python layer without a device, the declarations, and the
scoring and key functions of csrc/span_core.h -- what every lane of span_kernel runs -- start by start on the CPU under
AddressSanitizer + UBSan against the brute-force reference of tests/span_ref.py (tests/native/span_core.cpp)."""
import ctypes
import inspect
import os
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi
from tests.glob_ref import true_entries
from tests.span_ref import span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'pss_reader_match_spans'


def c_batch(patterns, offsets=None):
    blob = b''.join(patterns)
    offs = np.cumsum([0] + [len(t) for t in patterns]).astype(np.uint64) if offsets is None else np.array(offsets, dtype=np.uint64)
    return blob, offs


def test_einval_cases_with_a_null_reader():
    """Every malformed batch is reported as such without a reader, before the reader is looked at; out stays as it was."""
    fn = _ffi.lib.pss_reader_match_spans

    def refused(what, blob, offs, nq, ks, flags=0, id_offs=None, ids=(), out_ok=True, ids_ok=True, id_offs_ok=True):
        id_offs = np.array([0] * (nq + 1) if id_offs is None else id_offs, dtype=np.uint64)
        ids = np.array(ids, dtype=np.uint64)
        ks = None if ks is None else np.array(ks, dtype=np.uint8)
        out = np.full((max(ids.size, 1), 3), 7, dtype=np.int32)
        rc = fn(None, ids.ctypes.data if ids_ok else None, id_offs.ctypes.data if id_offs_ok else None, blob,
                None if offs is None else offs.ctypes.data, nq, None if ks is None else ks.ctypes.data, flags,
                out.ctypes.data if out_ok else None)
        assert rc == _ffi.PSS_EINVAL and (out == 7).all()
        assert NAME in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())

    for flags, unit in ((0, 'mismatches'), (1, 'edits'), (2, 'mismatches'), (3, 'edits')):
        blob, offs = c_batch([b'ab', b'', b'c'])
        refused('pattern 1 is empty', blob, offs, 3, [0, 0, 0], flags)
        blob, offs = c_batch([b'abcd', b'ab', b'abc'])
        refused('pattern 1 has 2 bytes and a budget of 2 %s' % unit, blob, offs, 3, [3, 2, 2], flags)
        refused('pattern 2 has 3 bytes and a budget of 3 %s' % unit, blob, offs, 3, [0, 1, 3], flags)
        refused('pattern 0 has a budget of 4 %s: 0 .. 3' % unit, blob, offs, 3, [4, 1, 1], flags)
        refused('pattern 2 has a budget of 255 %s' % unit, blob, offs, 3, [1, 1, 255], flags)
        refused('no reader', blob, offs, 3, [3, 1, 2], flags, id_offs=[0, 1, 1, 3], ids=[0, 1, 1 << 32])
    refused('start at 1, not at 0', *c_batch([b'ab', b'c'], [1, 2, 3]), 2, [0, 0])
    refused('decrease at pattern 1', *c_batch([b'abc', b'c'], [0, 3, 2]), 2, [0, 0])
    blob, offs = c_batch([b'ab', b'c'])
    for flags in (4, 8, 0x80000000, 7):
        refused('unknown flag bits', blob, offs, 2, [1, 0], flags)
    refused('the id offsets start at 1, not at 0', blob, offs, 2, [1, 0], id_offs=[1, 1, 1], ids=[0])
    refused('the id offsets decrease at pattern 1', blob, offs, 2, [1, 0], id_offs=[0, 2, 1], ids=[0, 0])
    refused('bad arguments', None, offs, 2, [1, 0])
    refused('bad arguments', blob, None, 2, [1, 0])
    refused('bad arguments', blob, offs, 2, None)
    refused('bad arguments', blob, offs, 2, [1, 0], id_offs_ok=False)
    refused('bad arguments', blob, offs, 2, [1, 0], id_offs=[0, 1, 2], ids=[0, 0], out_ok=False)
    refused('bad arguments', blob, offs, 2, [1, 0], id_offs=[0, 1, 2], ids=[0, 0], ids_ok=False)
    # what is malformed is named before the missing reader: the reader is judged last
    refused('no reader', blob, offs, 2, [1, 0])
    refused('no reader', b'', np.zeros(1, dtype=np.uint64), 0, [])
    refused('no reader', *c_batch([b'Error\n', b'12', b'abcdefghijklmnopqrstuvwxyz' * 8]), 3, [3, 1, 2], 3)


def test_python_argument_checks_need_no_reader():
    r = object.__new__(pss.Reader)
    ids, counts = np.array([0, 1, 2], dtype=np.uint64), np.array([2, 1], dtype=np.uint64)
    pats = [b'abcdefgh', b'PassWord']
    for edits in (False, True):
        with pytest.raises(ValueError, match='pattern 1 is empty'):
            r.match_spans_batch(ids, counts, [b'a', b''], 0, edits)
        with pytest.raises(ValueError, match='pattern 1 has 2 bytes and a budget of 2'):
            r.match_spans_batch(ids, counts, [b'abc', b'ab'], 2, edits)
        for bad in (4, -1, [1, 4]):
            with pytest.raises(ValueError, match='0 .. 3'):
                r.match_spans_batch(ids, counts, pats, bad, edits)
        with pytest.raises(ValueError, match='3 budgets for 2 patterns'):
            r.match_spans_batch(ids, counts, pats, [1, 1, 1], edits)
        for bad in (1, 0, None, 'yes', np.bool_(True)):
            with pytest.raises(TypeError, match='icase'):
                r.match_spans_batch(ids, counts, pats, 1, edits, icase=bad)
            with pytest.raises(TypeError, match='edits'):
                r.match_spans_batch(ids, counts, pats, 1, bad)
            with pytest.raises(TypeError, match='icase'):
                r.match_spans(ids, b'abcdefgh', 1, edits, icase=bad)
        with pytest.raises(TypeError):                       # keyword only
            r.match_spans_batch(ids, counts, pats, 1, edits, True)
        with pytest.raises(TypeError):
            r.match_spans(ids, b'abcdefgh', 1, edits, True)
        with pytest.raises(ValueError, match='the counts add up to 4 rows, ids has 3'):
            r.match_spans_batch(ids, [2, 2], pats, 1, edits)
        with pytest.raises(ValueError, match='the counts add up to 2 rows, ids has 3'):
            r.match_spans_batch(ids, [1, 1], pats, 1, edits)
        with pytest.raises(ValueError, match='3 counts for 2 patterns'):
            r.match_spans_batch(ids, [1, 1, 1], pats, 1, edits)
        with pytest.raises(ValueError, match='1 counts for 2 patterns'):
            r.match_spans_batch(ids, [3], pats, 1, edits)
    with pytest.raises(TypeError):
        r.match_spans_batch(ids, counts, b'abcdefgh', 1)     # one pattern in the place of a sequence
    with pytest.raises(TypeError):
        r.match_spans_batch(ids, counts, ['abcdefgh', 'x'], 0)
    with pytest.raises(TypeError):
        r.match_spans(ids, 7)
    with pytest.raises(TypeError):
        r.match_spans(ids, b'abcdefgh', True)
    with pytest.raises(TypeError):
        r.match_spans_batch(np.array([0.5, 1.0, 2.0]), counts, pats)
    with pytest.raises(ValueError, match='not negative'):
        r.match_spans_batch(np.array([0, -1, 2]), counts, pats)
    # every check passed: the closed reader is what is left to complain
    object.__setattr__(r, '_h', None)
    with pytest.raises(ValueError, match='closed Reader'):
        r.match_spans_batch(ids, counts, pats, [1, 2], True, icase=True)
    with pytest.raises(ValueError, match='closed Reader'):
        r.match_spans(ids, 'Password')


def test_declarations():
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert f'int {NAME}(' in hdr and 'typedef struct pss_span { int32_t start, length, distance; } pss_span;' in hdr
    assert '#define PSS_SPAN_EDITS 1u' in hdr and '#define PSS_SPAN_ICASE 2u' in hdr
    assert (_ffi.SPAN_EDITS, _ffi.SPAN_ICASE) == (1, 2)
    fn = getattr(_ffi.lib, NAME)                             # (exported: the loader resolved it)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [vp, vp, vp, vp, vp, u32, vp, u32, vp]
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    near = inspect.signature(pss.Reader.search_near_ids_batch).parameters
    for name, first in (('match_spans_batch', ['self', 'ids', 'counts', 'patterns']), ('match_spans', ['self', 'ids', 'pattern'])):
        line = next(ln for ln in stub.splitlines() if f'def {name}(' in ln)
        assert 'edits: bool = False, *, icase: bool = False' in line, name
        par = inspect.signature(getattr(pss.Reader, name)).parameters
        assert list(par) == first + ['k', 'edits', 'icase']
        for arg in ('k', 'edits', 'icase'):                  # search_near_ids_batch's, default for default
            assert par[arg].default == near[arg].default and par[arg].kind is near[arg].kind, (name, arg)
        assert 'start, length, distance' in getattr(pss.Reader, name).__doc__
    assert 'entry_bytes[start:start + length]' in pss.Reader.match_spans_batch.__doc__
    # no route bit and no environment switch of its own
    assert not any('SPAN' in name for name in _ffi.ROUTES) and 'PSS_SPAN_' not in hdr.replace('PSS_SPAN_EDITS', '').replace('PSS_SPAN_ICASE', '')


# ---- the scoring and key functions on the CPU ------------------------------------------------------------------------------------

ALPHABETS = (b'aAbB', b'\x00aA\xc1\xe1', b'ab', b'abcABC1', b'@`aA[{')


def random_case(rng):
    alpha = ALPHABETS[int(rng.integers(0, len(ALPHABETS)))]
    draw = lambda n: bytes(alpha[int(i)] for i in rng.integers(0, len(alpha), n))
    lengths = rng.choice([0, 1, 2, 3, 5, 8, 13, 30, 70, 140], int(rng.integers(1, 5)), p=[.1, .1, .1, .1, .15, .15, .1, .1, .07, .03])
    entries = [draw(int(n)) for n in lengths]
    closed = bool(rng.integers(0, 2)) or not entries[-1]
    text = b'\n'.join(entries) + (b'\n' if closed else b'')
    k = int(rng.integers(0, 4))
    line = int(rng.integers(0, len(entries)))
    e = entries[line]
    L = int(rng.choice([k + 1, k + 2, 4, 7, 8, 9, 16, 17]))
    L = max(L, k + 1)
    if len(e) >= L and rng.random() < 0.7:                   # cut from the entry, then up to k + 1 changes
        at = int(rng.integers(0, len(e) - L + 1))
        p = bytearray(e[at:at + L])
        for _ in range(int(rng.integers(0, k + 2))):
            op = int(rng.integers(0, 3))
            if op == 0:
                p.insert(int(rng.integers(0, len(p) + 1)), alpha[int(rng.integers(0, len(alpha)))])
            elif op == 1 and len(p) > k + 1:
                del p[int(rng.integers(0, len(p)))]
            else:
                p[int(rng.integers(0, len(p)))] = alpha[int(rng.integers(0, len(alpha)))]
        p = bytes(p)
    else:
        p = draw(L)
    if rng.random() < 0.15:                                  # ends in 0x00: the padding behind n must not match
        p = p[:-1] + b'\x00' if len(p) > 1 else p
    if rng.random() < 0.02:
        p = p[:len(p) // 2] + b'\n' + p[len(p) // 2 + 1:]
    return text, line, p, k, int(rng.integers(0, 4))


def test_the_scoring_functions_on_the_cpu(tmp_path):
    """About 5 000 random cases over small alphabets -- near matches and ties are the rule -- written with the reference's
    answer; the native program lays every text flush into a block with exactly the reader's padding behind n, runs
    span_core.h start by start as 64 lanes would, and compares.  Non-zero on a mismatch or a sanitizer report."""
    rng = np.random.default_rng(2020)
    fixed = [(b'ab\x00', 0, b'ab\x00\x00', 1, 0), (b'x\nab', 1, b'ab\x00', 1, 1), (b'ab', 0, b'abc', 1, 1), (b'a' * 70 + b'b', 0, b'ab', 0, 0),
             (b'passw0rd password', 0, b'password', 1, 3), (b'\n\nab\n', 1, b'ab', 1, 1), (b'ab\ncd', 0, b'abc', 1, 0)]
    blob, matched, kinds = [], 0, set()
    cases = fixed + [random_case(rng) for _ in range(5000)]
    for text, line, p, k, flags in cases:
        nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 0x0A)
        want = span(true_entries(text, nl)[line], p, k, bool(flags & 1), bool(flags & 2))
        matched += want[2] >= 0
        kinds.add((flags, want[2]))
        blob.append(struct.pack('<I', len(text)) + text + struct.pack('<II', line, len(p)) + p + struct.pack('<BBiii', k, flags, *want))
    assert matched > 1500 and kinds >= {(f, d) for f in range(4) for d in (-1, 0, 1, 2, 3)}
    path = tmp_path / 'cases.bin'
    path.write_bytes(struct.pack('<I', len(cases)) + b''.join(blob))
    csrc = os.path.join(ROOT, 'pysubstringsearch_amd', 'csrc')
    exe = str(tmp_path / 'span_core')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I' + csrc,
                        os.path.join(ROOT, 'tests', 'native', 'span_core.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'span_core: ok, %d cases' % len(cases) in r.stdout and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]
