"""tests/anchor_texts.py on the CPU: every generator at every size the GPU tests use (the construction checks run inside
the generators), the properties the anchor round's proof rests on (anchor_impl.h: M never decreases, every window holds an
anchor, the last position is one, M(s) - s depends on omega + w - 1 bytes only), and the numpy model against a plain double
loop that restates the kernel's definition position by position."""
import numpy as np
import pytest

from tests import anchor_texts as A

OMEGAS = (2, 8, 9, 16, 17, 64)
WS = (4, 8)
_TEXTS = {}


def _tiled(n, alpha):
    if (n, alpha) not in _TEXTS:
        t = A.tiled(n, alpha)
        t.setflags(write=False)
        _TEXTS[n, alpha] = t
    return _TEXTS[n, alpha]


def _loop_choices(codes, omega, w):
    """M(s) by the definition: hash every position, then look at every window."""
    n = len(codes)
    c = [int(v) for v in codes] + [0] * 8
    h = []
    for p in range(n):
        x = 0
        for j in range(w):
            x |= c[p + j] << (8 * j)
        h.append(((x * 0x9E3779B97F4A7C15) % (1 << 64)) >> 33)
    h += [0xffffffff] * omega
    out = []
    for s in range(n):
        best = s
        for q in range(s + 1, s + omega):
            if h[q] < h[best]:
                best = q
        out.append(best)
    return out


def _check_properties(t, omega, w, copies=None):
    codes = A.codes_of(t)
    n = t.size
    m = A.choices(codes, omega, w)
    s = np.arange(n)
    assert (m >= s).all() and (m < np.minimum(s + omega, n)).all()      # every window holds its anchor, inside the text
    assert (m[1:] >= m[:-1]).all()
    assert m[-1] == n - 1
    a = A.anchors(codes, omega, w)
    assert a.size == A.anchor_count(codes, omega, w) and a[-1] == n - 1
    assert (np.diff(a) <= omega).all() and a[0] < omega                 # no stretch of omega positions without one
    if copies:
        # locality: equal bytes for omega + w - 1 positions, equal M(s) - s -- over the copies of the block
        L, starts = copies
        span = L - (omega + w - 1) + 1
        if span > 0:
            d = m - s
            for b in starts[1:]:
                assert np.array_equal(d[starts[0]:starts[0] + span], d[b:b + span]), (omega, w, b)


@pytest.mark.parametrize('alpha', sorted(A.ALPHABETS))
def test_tiled_texts_and_the_proof_properties(alpha):
    for n in A.TILED_NS + (A.REFUSED_N,) + A.STALE_NS:
        t = _tiled(n, alpha)
        assert t.size == n and t.dtype == np.uint8
        for omega in OMEGAS:
            for w in WS:
                _check_properties(t, omega, w, A.copies_of_tiled(n))
    if alpha == 39:
        _check_properties(_tiled(A.LONG_N, alpha), 13, 4, A.copies_of_tiled(A.LONG_N))      # (the long text of the padding test)


def test_codes():
    t = _tiled(4096, 256)
    assert np.array_equal(A.codes_of(t), t)                              # all 256 byte values: raw bytes
    t = _tiled(4096, 4)
    assert sorted(set(A.codes_of(t).tolist())) == [1, 2, 3, 4, 5] and A.codes_of(t)[-1] == 1
    assert A.codes_of(np.frombuffer(b'zaza\n', dtype=np.uint8)).tolist() == [3, 2, 3, 2, 1]
    h = A.hashes(np.array([1, 2, 3, 4, 5], np.uint8), 4)
    assert int(h[0]) == ((0x04030201 * 0x9E3779B97F4A7C15) % (1 << 64)) >> 33
    assert int(h[3]) == ((0x0504 * 0x9E3779B97F4A7C15) % (1 << 64)) >> 33      # zero past the end
    h = A.hashes(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint8), 8)
    assert int(h[1]) == ((0x0908070605040302 * 0x9E3779B97F4A7C15) % (1 << 64)) >> 33
    assert int(h.max()) < A.ANC_HMAX


@pytest.mark.parametrize('w', WS)
@pytest.mark.parametrize('omega', OMEGAS)
def test_model_equals_the_double_loop(omega, w):
    rng = np.random.default_rng(omega * 10 + w)
    texts = [_tiled(65, 2), _tiled(64, 39), rng.integers(0, 2, 2000, dtype=np.uint8), rng.integers(0, 256, 1999, dtype=np.uint8),
             _tiled(4097, 4)[4097 - 1500:], np.zeros(300, np.uint8), np.resize(np.array([1, 2], np.uint8), 301)]
    for t in texts:
        codes = A.codes_of(t)
        assert A.choices(codes, omega, w).tolist() == _loop_choices(codes, omega, w)


def test_window_rule():
    assert A.window_of(10) == (7, 4) and A.window_of(27) == (24, 4) and A.window_of(28) == (21, 8)
    assert A.window_of(32, 9) == (9, 8) and A.window_of(12, 17) == (9, 4) and A.window_of(3) == (0, 4)
    assert A.window_of(70) == (63, 8) and A.window_of(71) == (64, 8) and A.window_of(96, 65) == (64, 8)
    assert A.runs(64, 2, 12) and not A.runs(63, 2, 12) and not A.runs(64, 1, 12)
    assert A.runs(100, 9, 20) and not A.runs(100, 9, 21) and A.runs(100, 9, 33, 3) and A.runs(100, 9, 33, 2)
    assert not A.runs(100, 9, 21, 7)                                     # (the knob clamps to 3 .. 5)


@pytest.mark.parametrize('div', A.CAP_DIVS)
def test_prefixes_on_the_cap(div):
    omega, on, over = A.on_the_cap(div, A.CAP_W)
    for t in (on, over):
        assert t[-1] == A.NL and t.size >= A.CAP_MIN
        L, starts = A.copies_of_tiled(A.CAP_N)
        assert sum(1 for s in starts if np.array_equal(t[s:s + L], A.cap_block(t))) >= 2      # two whole copies at least
    assert A.anchor_count(A.codes_of(on), omega, A.CAP_W) == on.size // div
    assert A.anchor_count(A.codes_of(over), omega, A.CAP_W) == over.size // div + 1
    assert A.runs(on.size, omega, on.size // div, div) and not A.runs(over.size, omega, over.size // div + 1, div)
    L, starts = A.copies_of_tiled(A.CAP_N)
    _check_properties(on, omega, A.CAP_W, (L, [s for s in starts if s + L < on.size]))


def test_ladder_drains(oracle):
    t = A.ladder()
    assert t.size <= 70000
    m = A.check_ladder(t, oracle.sa(t))
    print(m)
    _check_properties(t, 64, 8)


@pytest.mark.parametrize('alpha', A.DEEP_ALPHAS)
def test_deep(alpha):
    t = A.deep(A.DEEP_N, alpha)
    assert t.size == A.DEEP_N and t[-1] == A.NL
    assert np.unique(t).size == alpha + 1
    for omega, w in ((25, 8), (13, 4), (64, 8)):
        _check_properties(t, omega, w, A.copies_of_deep(A.DEEP_N, alpha))
