"""The host side of the search within k mismatches / k edits under ASCII case folding (include/pss.h, the three
pss_reader_*_near_icase_* calls and pss_near_seeds): no reader, no GPU.  The rule sets the kernels
implement, restated hit by hit (tests/near_icase_ref.py), are held against the brute force; the expansion the C layer
performs (near_seeds) against the restated seed rule; the request rule against csrc/search_layout.h on the CPU; then the
argument checks of the C calls without a reader and of the Python layer without a device, and the declarations."""
import ctypes
import inspect
import os
import pathlib
import subprocess

import numpy as np
import pytest

import pysubstringsearch_amd as pss
from pysubstringsearch_amd import _ffi
from tests import near_icase_ref as nir
from tests.edit_ref import EditRef
from tests.near_icase_ref import CAP, EditIcaseRef, NearIcaseRef
from tests.near_ref import NearRef, pieces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_CALLS = ('pss_reader_search_near_icase_batch', 'pss_reader_search_near_icase_ids_batch', 'pss_reader_count_near_icase_batch')
METHODS = ('search_near_batch_packed', 'search_near_ids_batch', 'count_near_bytes', 'search_near', 'count_near')
# both cases of two letters, a digit, the bytes that sit one below `A` / `a`, a newline and a letter outside ASCII
ALPHABET = np.frombuffer(b'aAbB1@`\xe9\n', np.uint8)


def random_case(rng):
    pr = np.r_[np.full(4, 1.0), 0.4, 0.25, 0.25, 0.3, 0.6]
    text = bytes(ALPHABET[rng.choice(len(ALPHABET), int(rng.integers(1, 48)), p=pr / pr.sum())])
    k = int(rng.integers(0, 4))
    pp = pr[:-1] / pr[:-1].sum()
    p = bytes(ALPHABET[rng.choice(len(ALPHABET) - 1, int(rng.integers(k + 1, 9)), p=pp)])
    return text, p, k, int(rng.integers(1, 7))


@pytest.mark.parametrize('edits', [False, True], ids=['mismatches', 'edits'])
def test_the_rule_set_of_the_kernels_agrees_with_the_brute_force(edits):
    """Seed hits, the whole piece under fold, the earlier pieces, the budget, the entry and the leftward dedupe, restated on
    the CPU, keep exactly one hit per matching entry and leave them in the stated order: 1 600 random small cases per kind,
    every k, seed letters 1 .. 6, newlines inside the text, pieces over the letter cap, and the relations of the contract
    beside them -- the fold answer contains the exact one, the edits answer the mismatch answer, k = 0 is the
    case-insensitive answer."""
    rng = np.random.default_rng(1910 + edits)
    ref_cls, rules = (EditIcaseRef, nir.edit_rule_set_lines) if edits else (NearIcaseRef, nir.rule_set_lines)
    fixed = [(b'AbaB\nabb\nBAB\naab\nAb\n', b'abAB', 1, 1), (b'aAb\nab\nAA\nb\nabaAB', b'AaB', 1, 2), (b'aB\nAb\n', b'abab', 1, 5),
             (b'a\nB', b'Ab', 1, 5), (b'@a`\n`A@', b'@A@', 1, 3)]
    matched = more = over_cap = inner = 0
    for i in range(1600):
        text, p, k, letters = fixed[i] if i < len(fixed) else random_case(rng)
        ref = ref_cls([text])
        ref.letters = letters
        find = ref.search_edit_ids if edits else ref.search_near_ids
        want = ref.ordered_ids(p, k).tolist()
        assert rules(text, p, k, letters) == want, (text, p, k, letters)
        ids = find(p, k).tolist()
        assert sorted(want) == ids and len(set(want)) == len(want)
        exact = (EditRef([text]).search_edit_ids(p, k) if edits else NearRef([text]).search_near_ids(p, k)).tolist()
        assert set(exact) <= set(ids), (text, p, k)
        if edits:
            assert set(NearIcaseRef([text]).search_near_ids(p, k).tolist()) <= set(ids), (text, p, k)
        if k == 0:
            assert ids == [line for line, e in enumerate(ref._true[0]) if b'\n' not in p and p.lower() in e.lower()]
        matched += len(ids)
        more += len(ids) > len(exact)
        f = min(letters, CAP[k])
        over = [sum(map(nir.is_letter, piece)) > f for _, piece in pieces(p, k)]
        over_cap += any(over)
        inner += any(o and nir.fold_seed(piece, f)[0] > 0 for o, (_, piece) in zip(over, pieces(p, k)))
    assert matched > 1000 and more > 300 and over_cap > 300 and inner > 50, (matched, more, over_cap, inner)


def test_examples_of_the_contract():
    text = b'Password\npassw0rd\nPASSW0RD\nPASWORD\npass\nWORD\n`assword\nP@SSWORD\n\xc9t\xe9\n\xe9T\xe9'
    near, edit = NearIcaseRef([text]), EditIcaseRef([text])
    assert NearRef([text]).search_near_ids(b'Password', 1).tolist() == [0, 6]
    assert near.search_near_ids(b'Password', 0).tolist() == [0]
    assert near.search_near_ids(b'Password', 1).tolist() == [0, 1, 2, 6, 7]
    assert edit.search_edit_ids(b'Password', 1).tolist() == [0, 1, 2, 3, 6, 7]
    # nothing but A-Z folds: 0xC9 / 0xE9 differ, and so do the bytes one below the letters
    assert near.search_near_ids(b'\xe9t\xe9', 0).tolist() == [9] and near.search_near_ids(b'\xe9t\xe9', 1).tolist() == [8, 9]
    assert near.search_near_ids(b'`', 0).tolist() == [6] and near.search_near_ids(b'@', 0).tolist() == [7]
    assert near.search_near_ids(b'pass\nword', 1).size == 0 and near.piece_hits(b'pass\nword', 1) == 0
    # hits: every spelling of every piece's seed, exact
    assert near.piece_hits(b'ab1', 0) == sum(text.count(s) for s in (b'AB1', b'Ab1', b'aB1', b'ab1'))


# ---- the expansion: near_seeds against the restated rule ---------------------------------------------------------------------

def test_near_seeds_restates_the_seed_rule():
    rng = np.random.default_rng(1920)
    pats = [b'Password', b'abcdefghijklmn', b'12345678', b'a', b'ab1', b'AbaB', b'aAb', b'@`[{', b'1a2b3c4d5e6f7g8h', b'\xc9t\xe9X\x00y']
    pats += [bytes(ALPHABET[rng.integers(0, len(ALPHABET) - 1, int(rng.integers(1, 30)))]) for _ in range(60)]
    pats += [bytes(rng.integers(0x41, 0x7b, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(40)]
    most = 0
    for p in pats:
        for k in range(min(4, len(p))):
            for letters in (None, 1, 2, 3, 4, 5, 6):
                got = pss.near_seeds(p, k, letters)
                assert got == nir.seeds(p, k, nir.LETTERS if letters is None else letters), (p, k, letters)
                assert 1 <= len(got) <= 64
                most = max(most, len(got))
                cut = pieces(p, k)
                assert [j for j, _, _ in got] == sorted(j for j, _, _ in got) and {j for j, _, _ in got} == set(range(k + 1))
                for j, pos, q in got:       # every query is a spelling of a window of its piece, where it stands in the pattern
                    off, piece = cut[j]
                    assert off <= pos and pos + len(q) <= off + len(piece) and q.lower() == p[pos:pos + len(q)].lower()
                if k == 0:                  # exactly the queries of the case-insensitive search
                    seed_off, variants = pss.icase_variants(p, letters)
                    assert [q for _, _, q in got] == variants and {pos for _, pos, _ in got} == {seed_off}
    assert most == 64
    # a piece with more letters than the cap gets an inner seed: 14 letters at k = 1 are two pieces of 7, the cap is 5
    got = pss.near_seeds(b'abcdefghijklmn', 1)
    assert len(got) == 64 and got[0] == (0, 0, b'ABCDE') and got[31] == (0, 0, b'abcde') and got[32] == (1, 7, b'HIJKL')
    got = pss.near_seeds(b'1abcdefg', 0, 6)
    assert got[0][:2] == (0, 0) and len(got[0][2]) == 7                     # (leftmost on a tie)
    got = pss.near_seeds(b'abcdefg1', 0, 6)
    assert got[0][:2] == (0, 1) and len(got[0][2]) == 7 and len(got) == 64  # (the longest window stands inside)
    assert pss.near_seeds(b'12345678', 3) == [(0, 0, b'12'), (1, 2, b'34'), (2, 4, b'56'), (3, 6, b'78')]
    for k, cap in enumerate(CAP):           # the cap is the largest f with (k + 1) 2^f <= 64
        assert (k + 1) << cap <= 64 < (k + 1) << (cap + 1)
        assert len(pss.near_seeds(b'abcdefgh' * 4, k, 6)) == (k + 1) << cap


def test_near_seeds_argument_checks():
    with pytest.raises(TypeError):
        pss.near_seeds('abc', 1)
    with pytest.raises(TypeError):
        pss.near_seeds(b'abc', True)
    for bad in (4, -1):
        with pytest.raises(ValueError, match='0 .. 3'):
            pss.near_seeds(b'abcdefgh', bad)
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match='letters'):
            pss.near_seeds(b'abcdefgh', 1, bad)
    with pytest.raises(ValueError):
        pss.near_seeds(b'', 0)
    with pytest.raises(ValueError):
        pss.near_seeds(b'ab', 2)
    lib, u32 = _ffi.lib, ctypes.c_uint32
    piece, pos, ln, cnt = (u32 * 64)(), (u32 * 64)(), (u32 * 64)(), u32()
    assert lib.pss_near_seeds(b'abcd', 4, 1, 0, None, 0, piece, pos, ln, None) == _ffi.PSS_EINVAL
    assert lib.pss_near_seeds(b'abcd', 4, 1, 7, None, 0, piece, pos, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert lib.pss_near_seeds(b'abcd', 4, 4, 0, None, 0, piece, pos, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert lib.pss_near_seeds(b'abcd', 4, 1, 0, None, 0, piece, pos, ln, ctypes.byref(cnt)) == _ffi.PSS_OK and cnt.value == 8
    buf = ctypes.create_string_buffer(16)
    assert lib.pss_near_seeds(b'abcd', 4, 1, 0, buf, 15, piece, pos, ln, ctypes.byref(cnt)) == _ffi.PSS_EINVAL
    assert 'more than the 15 bytes of out' in _ffi.last_error() and cnt.value == 8
    assert lib.pss_near_seeds(b'abcd', 4, 1, 0, buf, 16, piece, pos, ln, ctypes.byref(cnt)) == _ffi.PSS_OK
    assert buf.raw == b'ABAbaBabCDCdcDcd' and list(piece[:8]) == [0] * 4 + [1] * 4 and list(pos[:8]) == [0] * 4 + [2] * 4


# ---- the request rule on the CPU -----------------------------------------------------------------------------------------------

def test_the_request_rule_on_the_cpu(tmp_path):
    """tests/native/near_fold_request.cpp against csrc/search_layout.h alone, under AddressSanitizer + UBSan: one valid
    fold-near and one valid fold-edit request, every new clause broken (near_fold without budgets, with sequence anchors,
    with a term that excludes, with a class block), and the sizes of a seeded layout with budgets written out."""
    csrc = os.path.join(ROOT, 'pysubstringsearch_amd', 'csrc')
    exe = str(tmp_path / 'near_fold_request')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I' + csrc,
                        os.path.join(ROOT, 'tests', 'native', 'near_fold_request.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'near_fold_request: ok' in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


# ---- the argument checks of the three calls, without a reader ------------------------------------------------------------------

def c_batch(patterns, offsets=None):
    blob = b''.join(patterns)
    offs = np.cumsum([0] + [len(t) for t in patterns]).astype(np.uint64) if offsets is None else np.array(offsets, dtype=np.uint64)
    return blob, offs


@pytest.mark.parametrize('edits', [0, 1], ids=['mismatches', 'edits'])
def test_einval_cases_with_a_null_reader(edits):
    """Every malformed batch is reported as such without a reader, in near's words and order; the null reader is judged last."""
    lib = _ffi.lib
    searches = (lib.pss_reader_search_near_icase_batch, lib.pss_reader_search_near_icase_ids_batch)
    unit = 'edits' if edits else 'mismatches'

    def refused(what, blob, offs, nq, ks, out_ok=True):
        offs_p = None if offs is None else offs.ctypes.data
        ks = None if ks is None else np.array(ks, dtype=np.uint8)
        ks_p = None if ks is None else ks.ctypes.data
        for fn in searches:
            out = ctypes.c_void_p()
            assert fn(None, blob, offs_p, nq, ks_p, edits, ctypes.byref(out) if out_ok else None) == _ffi.PSS_EINVAL
            assert not out.value and fn.__name__ in _ffi.last_error() and what in _ffi.last_error(), (what, _ffi.last_error())
        counts = np.full(4, 7, dtype=np.uint64)
        assert lib.pss_reader_count_near_icase_batch(None, blob, offs_p, nq, ks_p, edits, counts.ctypes.data if out_ok else None) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pss_reader_count_near_icase_batch' in _ffi.last_error() and what in _ffi.last_error()

    blob, offs = c_batch([b'ab', b'', b'c'])
    refused('pattern 1 is empty', blob, offs, 3, [0, 0, 0])
    blob, offs = c_batch([b'abcd', b'ab', b'abc'])
    refused('pattern 1 has 2 bytes and a budget of 2 %s' % unit, blob, offs, 3, [3, 2, 2])
    refused('pattern 2 has 3 bytes and a budget of 3 %s' % unit, blob, offs, 3, [0, 1, 3])
    refused('pattern 0 has a budget of 4 %s: 0 .. 3' % unit, blob, offs, 3, [4, 1, 1])
    refused('pattern 2 has a budget of 255 %s' % unit, blob, offs, 3, [1, 1, 255])
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


def test_python_argument_checks_need_no_reader():
    args = pss.Reader._near_args
    for edits in (False, True):
        blob, offs, ks = args([b'PassWord', b'ab'], 1, edits, icase=True)
        assert bytes(blob) == b'PassWordab' and offs.tolist() == [0, 8, 10] and ks.dtype == np.uint8 and ks.tolist() == [1, 1]
        with pytest.raises(ValueError, match='pattern 1 is empty'):
            args([b'a', b''], 0, edits, icase=True)
        with pytest.raises(ValueError, match='pattern 1 has 2 bytes and a budget of 2'):
            args([b'abc', b'ab'], 2, edits, icase=True)
        for bad in (4, -1, [1, 4]):
            with pytest.raises(ValueError, match='0 .. 3'):
                args([b'abcdefgh', b'abcdefgh'], bad, edits, icase=True)
        for bad in (1, 0, None, 'yes', [True], np.bool_(True)):
            with pytest.raises(TypeError, match='icase'):
                args([b'abcdefgh'], 1, edits, icase=bad)
    # the keyword reaches the check from every method, before a reader is asked for anything
    r = object.__new__(pss.Reader)
    for name in METHODS:
        first = 'abcdefgh' if name in ('search_near', 'count_near') else [b'abcdefgh']
        with pytest.raises(TypeError, match="argument 'icase' must be a bool"):
            getattr(r, name)(first, 1, icase=1)
        with pytest.raises(TypeError):                   # keyword only
            getattr(r, name)(first, 1, False, True)


def test_declarations():
    hdr = pathlib.Path(os.path.join(ROOT, 'include', 'pss.h')).read_text()
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    for name in C_CALLS + ('pss_near_seeds',):
        assert f'int {name}(' in hdr, f'{name} is not declared in include/pss.h'
        fn = getattr(_ffi.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, f'{name} has no argument types in _ffi.py'
    assert list(_ffi.lib.pss_reader_search_near_icase_batch.argtypes) == [vp, vp, vp, u32, vp, ci, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_search_near_icase_ids_batch.argtypes) == [vp, vp, vp, u32, vp, ci, ctypes.POINTER(vp)]
    assert list(_ffi.lib.pss_reader_count_near_icase_batch.argtypes) == [vp, vp, vp, u32, vp, ci, vp]
    stub = pathlib.Path(os.path.join(ROOT, 'pysubstringsearch_amd', '__init__.pyi')).read_text()
    assert 'def near_seeds(pattern: bytes, k: int, letters: typing.Optional[int] = None)' in stub and 'near_seeds' in pss.__all__
    for name in METHODS:
        assert '*, icase: bool = False' in next(ln for ln in stub.splitlines() if f'def {name}(' in ln), name
        par = inspect.signature(getattr(pss.Reader, name)).parameters['icase']
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY, name
        assert 'icase=True' in getattr(pss.Reader, name).__doc__, name
    # no route bit and no environment switch of its own
    assert not any('FOLD' in name or 'ICASE' in name for name in _ffi.ROUTES) and 'PSS_NEAR_ICASE' not in hdr
