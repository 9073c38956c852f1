"""The LSD radix sort (radix_sort.hip) on its edges, every result compared for EQUALITY with the numpy model of
tests/lsd_texts.py: the (key, value) passes on both sides of the one-tile sort and of every range geometry, the
flag-carrying passes of the initial suffix sort on texts that walk each of the five routes a tie flag can take (checked
on the CPU by tests/test_lsd_texts.py) at every key width and every prefix of a run, the end of the text, the plain
passes over the text, the geometry every build uses, and the route a whole build takes.  The range cap of 8
(pss_sort_pairs_ex_device / pss_suffix_sort_device) makes a range hold three or four tiles at 10^5 elements; no build
ever lowers it."""
import numpy as np
import pytest
import torch

from pysubstringsearch_amd import _ffi
from tests import lsd_texts as L
from tests.util import sa_device

pytestmark = pytest.mark.gpu

_CACHE = {}
DEFAULT = L.RS_MAX_RANGES


def _cached(key, make):
    """Texts, keys and model answers: made once per session, never written to."""
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


# ---- a. (key, value) pairs -------------------------------------------------------------------------------------------

def _sort_pairs(keys, vals, key_bits, mask, cap):
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.from_numpy(vals.view(np.int32).copy()).cuda()
    _ffi.check(_ffi.lib.pss_sort_pairs_ex_device(dk.data_ptr(), dv.data_ptr(), keys.size, key_bits, mask, cap, 0))
    return dk.cpu().numpy().view(np.uint64), dv.cpu().numpy().view(np.uint32)


def _keys(shape, n, key_bits, rng):
    """Keys of one shape in the digits the sort looks at, random bits in every byte above them."""
    full = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if shape == 'uniform':
        return full
    if shape == 'third':
        k = full.copy()
        k[rng.random(n) < 1 / 3] = np.uint64(0x5a5a5a5a5a5a5a5a)
    elif shape == 'equal':
        k = np.full(n, 0xc3c3c3c3c3c3c3c3, dtype=np.uint64)
    elif shape == 'sorted':
        k = np.sort(rng.integers(0, 8, n).astype(np.uint64)) * np.uint64(0x0101010101010101)
    elif shape == 'two':
        k = np.zeros(n, dtype=np.uint64)
        for p in range(8):
            pair = rng.integers(0, 256, 2).astype(np.uint64)
            k |= pair[rng.integers(0, 2, n)] << np.uint64(8 * p)
    elif shape == 'ones':       # the one-tile sort pads with key ~0, value ~0: real all-ones keys must stay in front of it
        k = np.where(rng.random(n) < 0.5, np.uint64(0xffffffffffffffff), full)
    else:
        raise ValueError(shape)
    above = 8 * L.passes_of(key_bits)
    if above < 64:
        k = (k & L._low(above)) | (full & ~L._low(above))
    return k


PAIR_SIZES = [(n, DEFAULT) for n in (1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 8 * 4096, 8 * 4096 + 1)] + \
             [(n, 8) for n in (4097, 8193, 8 * 4096, 8 * 4096 + 1, 3 * 8 * 4096, 3 * 8 * 4096 + 1, 69631)]
KEY_BITS = (1, 8, 9, 17, 33, 41, 64)
# (key_bits, pass_mask): every pass, the run-length path's call, the first pass skipped, a single pass
MASKS = ((41, 0x3f), (33, 0xfffffffe), (64, 0x04))


@pytest.mark.parametrize('n,cap', PAIR_SIZES)
def test_pairs_against_the_stable_sort(n, cap):
    """Keys AND values at every size: one element, both sides of the one-tile sort (4096) and of two tiles, the largest n
    with one tile per range at cap 8 and the first with two (a last range of one element, three empty ranges), three
    and four tiles per range, a last tile of 4095.  Values are arange, so the one-tile sort's (key, value) order IS the
    stable order.  Every key width with uniform keys (random above the digits sorted by, which the sort must ignore), the
    other shapes at 17 and 64 bits, and the pass masks."""
    rng = np.random.default_rng(n * 31 + cap)
    vals = np.arange(n, dtype=np.uint32)
    runs = [('uniform', kb, 0xffffffff) for kb in KEY_BITS]
    runs += [(s, kb, 0xffffffff) for s in ('third', 'equal', 'sorted', 'two', 'ones') for kb in (17, 64)]
    runs += [(s, kb, m) for s in ('uniform', 'third', 'two') for kb, m in MASKS]
    for shape, kb, mask in runs:
        keys = _keys(shape, n, kb, rng)
        wk, wv = L.want_pairs(keys, vals, kb, mask)
        gk, gv = _sort_pairs(keys, vals, kb, mask, cap)
        note = (shape, kb, hex(mask), n, L.geometry(n, cap))
        assert np.array_equal(gv, wv), (note, 'first wrong value at', int(np.flatnonzero(gv != wv)[0]))
        assert np.array_equal(gk, wk), note


def test_pairs_reject_a_bad_cap():
    d = torch.zeros(16, dtype=torch.int64, device='cuda')
    v = torch.zeros(16, dtype=torch.int32, device='cuda')
    for cap in (0, 4, 12, 1032, 2048):
        assert _ffi.lib.pss_sort_pairs_ex_device(d.data_ptr(), v.data_ptr(), 16, 64, 0xff, cap, 0) == _ffi.PSS_EINVAL


# ---- b .. e. the passes over the text --------------------------------------------------------------------------------

def _suffix_sort(codes, n, cfg, key_bits, flags, cap):
    b, k, drop, plus_one = cfg
    d = torch.from_numpy(np.array(codes)).cuda()          # (a copy: the cached text is read-only)
    assert d.data_ptr() % 16 == 0 and d.numel() >= n + L.PAD
    out = torch.empty(n, dtype=torch.int32, device='cuda')
    _ffi.check(_ffi.lib.pss_suffix_sort_device(d.data_ptr(), n, b, k, plus_one, drop, key_bits, 1 if flags else 0, cap,
                                               out.data_ptr(), 0))
    return out.cpu().numpy().view(np.uint32)


def _planted(cfg, n):
    def make():
        b, k, drop, plus_one = cfg
        codes = L.padded(L.planted(cfg, n), plus_one)
        return codes, L.pack_keys(codes, n, b, k, plus_one, drop)
    return _cached(('planted', cfg, n), make)


def _compare(got, keys, key_bits, flags, cap, note):
    want = L.want_suffix(keys, key_bits, flags)
    if np.array_equal(got, want):
        return
    at = int(np.flatnonzero(got != want)[0])
    lines = ['%r key_bits %d flags %d: first wrong position %d: got %#x, want %#x; geometry %r' %
             (note, key_bits, flags, at, int(got[at]), int(want[at]), L.geometry(keys.size, cap))]
    elem = int(want[at] & 0x7fffffff)
    for p, (out, route, tied) in enumerate(L.replay(keys, key_bits, cap)):
        j = int(np.flatnonzero((out & 0x7fffffff) == elem)[0])
        lines.append('  pass %d: element %d lands at %d by %s, tied %d' %
                     (p, elem, j, L.ROUTES[route[j]] if route[j] >= 0 else 'first of its digit', int(tied[j])))
    raise AssertionError('\n'.join(lines))


@pytest.mark.parametrize('cfg', L.CONFIGS)
def test_flag_passes_at_a_small_cap(cfg):
    """suffix_sort_flags with three and four tiles per range on the planted texts: indices and bit 31 element by element.
    The widest key of every code width also runs at every prefix of its passes, 9 .. 64 bits -- all six key-plane
    instantiations, and no wrong intermediate flag can hide behind the later digits.  The 64 bytes past the end of a
    plus_one text hold 0xFF: only the kernels' own bounds keep them out of the keys."""
    for n in L.PLANTED_NS:
        codes, keys = _planted(cfg, n)
        for kb in L.sweep_of(cfg):
            _compare(_suffix_sort(codes, n, cfg, kb, True, L.CAP), keys, kb, True, L.CAP, (cfg, n))


@pytest.mark.parametrize('cap', [L.CAP, DEFAULT])
def test_text_tail(cap):
    """n mod 16 = 0, 1, 15 and a tied group whose last, cut copy has a key that goes on 0, 1, 7, 8, 15, 16 symbols past the
    end of the text (as far as the key is long): the zero padding is part of that key."""
    for cfg in L.TAIL_CONFIGS:
        b, k, drop, plus_one = cfg
        for n in L.TAIL_NS:
            for reach in L.TAIL_REACH:
                if reach > k:
                    continue
                codes = L.padded(L.tail_case(n, cfg, reach)[0], plus_one)
                keys = L.pack_keys(codes, n, b, k, plus_one, drop)
                for flags in (True, False):
                    got = _suffix_sort(codes, n, cfg, L.key_width(cfg), flags, cap)
                    _compare(got, keys, L.key_width(cfg), flags, cap, (cfg, n, reach))


@pytest.mark.parametrize('cfg', L.NO_FLAGS_CONFIGS)
def test_plain_passes_over_the_text(cfg):
    """radix_sort_pairs with the text as its source (the route of PSS_NO_TIES_PASS) on the same texts: plain indices, at
    the full width and at one digit."""
    for n in L.PLANTED_NS:
        codes, keys = _planted(cfg, n)
        for kb in (L.key_width(cfg), 8):
            _compare(_suffix_sort(codes, n, cfg, kb, False, L.CAP), keys, kb, False, L.CAP, (cfg, n))


def test_the_geometry_every_build_uses():
    """The default cap at n = 2^22 + 1: 1025 tiles, two per range, 513 ranges in use of 520, the last of them holding one
    element.  A skewed text, a 55-bit key, with flags and without."""
    cfg, n = (6, 10, 5, 0), (1 << 22) + 1
    assert L.geometry(n) == (1025, 2, 520) and L.key_width(cfg) == 55
    codes = L.padded(L.skewed(n, 6, 0), 0)
    keys = L.pack_keys(codes, n, *cfg[:2], cfg[3], cfg[2])
    for flags in (True, False):
        got = _suffix_sort(codes, n, cfg, 55, flags, DEFAULT)
        assert np.array_equal(got, L.want_suffix(keys, 55, flags)), flags


def test_suffix_sort_rejects_bad_arguments():
    d = torch.zeros(256, dtype=torch.uint8, device='cuda')
    out = torch.zeros(64, dtype=torch.int32, device='cuda')

    def rc(b=8, k=8, plus_one=0, drop=0, kb=64, flags=1, cap=8, ptr=None):
        return _ffi.lib.pss_suffix_sort_device(d.data_ptr() if ptr is None else ptr, 64, b, k, plus_one, drop, kb, flags, cap,
                                               out.data_ptr(), 0)
    assert rc() == _ffi.PSS_OK
    for bad in (dict(kb=8), dict(kb=65), dict(kb=0, flags=0), dict(k=0), dict(k=17, b=2, kb=16), dict(b=9, k=8), dict(drop=8),
                dict(drop=1, kb=64), dict(cap=12), dict(ptr=d.data_ptr() + 8)):
        assert rc(**bad) == _ffi.PSS_EINVAL, bad


# ---- f. the route of a whole build -----------------------------------------------------------------------------------

def _build_text(which):
    if which == 0:
        return L.planted((4, 16, 3, 0), 98305)
    if which == 1:
        return L.planted((6, 10, 5, 0), 69631)
    t = L.planted((9, 7, 0, 1), 65537).copy()
    t[:256] = np.arange(256, dtype=np.uint8)           # every byte value: 9-bit codes, symbol = byte + 1
    return t


@pytest.mark.parametrize('which,drop_last', [(0, True), (1, False), (2, True)])
def test_model_against_a_whole_build(oracle, monkeypatch, which, drop_last):
    """A whole build forced onto the LSD passes (no MSD sort, no sample sort, no run-length path, no closed form) with the
    key forced as wide as it goes: as many passes as the key has digits, the suffix array equal to the oracle's -- and the
    model's keys, packed from the text the way the hook is told to pack them, never decrease along that suffix array."""
    t = _cached(('build', which), lambda: np.ascontiguousarray(_build_text(which)))
    want = _cached(('build sa', which), lambda: oracle.sa(t))
    sigma = int(np.unique(t).size)
    plus_one = 1 if sigma == 256 else 0
    b = 9 if plus_one else max(1, sigma.bit_length())
    k = min(16, 64 // b)
    drop = b - 1 if drop_last else 0
    for name, v in dict(PSS_MSD=0, PSS_SS=0, PSS_RLE=0, PSS_PERIOD=0, PSS_KEY_CHARS=k, PSS_KEY_DROP=drop).items():
        monkeypatch.setenv(name, str(v))
    st = {}
    sa = sa_device(np.array(t), st)               # (a copy: the cached text is read-only)
    assert np.array_equal(sa, want)
    assert (st['code_bits'], st['key_chars'], st['key_bits']) == (b, k, k * b - drop)
    assert st['initial_passes'] == (st['key_bits'] + 7) // 8 and (st['msd'], st['ss'], st['rle']) == (0, 0, 0)
    # the hook on the same key: dense codes in byte order (raw bytes when all 256 occur)
    codes = t if plus_one else (np.searchsorted(np.unique(t), t) + 1).astype(np.uint8)
    codes = L.padded(codes, plus_one)
    keys = L.pack_keys(codes, t.size, b, k, plus_one, drop)
    along = keys[sa.astype(np.int64)]
    assert (along[1:] >= along[:-1]).all()
    cfg = (b, k, drop, plus_one)
    _compare(_suffix_sort(codes, t.size, cfg, k * b - drop, True, DEFAULT), keys, k * b - drop, True, DEFAULT, ('build', which))
