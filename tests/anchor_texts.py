"""The anchor round (csrc/anchor_impl.h, AnchorRound in csrc/anchor_driver_impl.h) restated in numpy, and the texts that
put it on its edges (tests/test_anchor_edges_gpu.py).  Everything here runs on the CPU; tests/test_anchor_texts.py runs
every generator for every size the GPU tests use and holds the model to a plain double loop.

The model:
  codes_of(t)        bytes -> dense codes 1 .. sigma in byte order (all 256 byte values present: the raw bytes)
  hashes(codes, w)   H(p) = ((x * 0x9E3779B97F4A7C15) mod 2^64) >> 33, x = the w code bytes at p, little-endian, zero past n
  choices(...)       M(s) = the LEFTMOST position of the smallest H in [s, s + omega), positions >= n count as 0xffffffff
  anchors(...)       the distinct values of M;  anchor_count(...)  their number
  window_of(...)     the host's rule for (omega, w) from the depth the build has reached;  runs(...)  whether the round is taken

The texts: uniform fill with non-periodic copies of one block (no two windows of `gram` symbols of the block are equal),
separated by fresh fill of differing lengths -- the suffixes inside the copies stay tied far past any text round, which
is what sends a build to the anchor round.
  tiled(n, alpha)   copies across the border of a tile of ANC_TILE window starts and up to the last byte before the newline
  ladder()          2-bit codes, words of 24 .. 88 bytes with copy counts falling with their length: every text round
                    resolves more than 40 % of what the one before left, so the build gets deep enough for the widest window
  on_the_cap(div)   two prefixes of one text whose anchors number exactly n // div and n // div + 1
  deep(n, alpha)    copies of n / 8 bytes: the anchors' names repeat as well, and a second level of anchors goes on top"""
import collections

import numpy as np

from tests.sa_edge_texts import FILL39, NL, count_sharing

ANC_TILE = 4096
ANC_HMAX = 0xffffffff
ANC_MULT = 0x9E3779B97F4A7C15
OMEGA_MAX = 64
MIN_N = 64

ALPHABETS = {2: b'ab', 4: b'acgt', 39: FILL39, 256: bytes(range(256))}
TILED_NS = (64, 65, 4095, 4096, 4097, 4111, 4112, 4113, 8191, 8193, 3 * 4096 + 5)
REFUSED_N = 63
STALE_NS = (4097, 4105, 4111)                 # n % 16 = 1, 9, 15
LONG_N = 70001                                # the text built before them, on the same context
CAP_DIVS = (3, 4, 5)
CAP_OMEGAS = {3: (5, 6, 4, 7), 4: (7, 8, 6, 9), 5: (9, 10, 11)}      # windows whose density 2 / (omega + 1) sits near 1 / div, best first
DEEP_ALPHAS = (4, 39)

Window = collections.namedtuple('Window', 'omega w')


# ---- the model -------------------------------------------------------------------------------------------------------

def codes_of(t):
    t = np.ascontiguousarray(t, dtype=np.uint8)
    present = np.unique(t)
    if present.size == 256:
        return t.copy()
    lut = np.zeros(256, np.uint8)
    lut[present] = np.arange(1, present.size + 1, dtype=np.uint8)
    return lut[t]


def hashes(codes, w):
    assert w in (4, 8)
    n = len(codes)
    c = np.concatenate([np.asarray(codes, dtype=np.uint64), np.zeros(8, np.uint64)])
    x = np.zeros(n, np.uint64)
    for j in range(w):
        x |= c[j:j + n] << np.uint64(8 * j)
    return (x * np.uint64(ANC_MULT)) >> np.uint64(33)          # (the product wraps at 2^64)


def choices(codes, omega, w):
    n = len(codes)
    assert n >= 1 and omega >= 1
    h = np.concatenate([hashes(codes, w), np.full(omega, ANC_HMAX, np.uint64)])
    key = (h << np.uint64(32)) | np.arange(n + omega, dtype=np.uint64)      # smallest H first, then the smallest position
    best = key[:n].copy()
    for q in range(1, omega):
        np.minimum(best, key[q:q + n], out=best)
    return (best & np.uint64(0xffffffff)).astype(np.int64)


def anchors(codes, omega, w):
    return np.unique(choices(codes, omega, w))


def anchor_count(codes, omega, w):
    m = choices(codes, omega, w)
    return 1 + int(np.count_nonzero(m[1:] != m[:-1]))            # (M never decreases: the distinct values are the changes)


def window_of(depth, forced=None, level0=True):
    """(omega, w) of AnchorRound::window for a text whose tied suffixes share `depth` symbols; forced: PSS_ANCHOR_OMEGA."""
    assert level0
    w = 8 if depth >= 28 else 4
    omega = depth - w + 1 if depth >= w else 0
    if forced:
        omega = min(omega, int(forced))
    return Window(min(omega, OMEGA_MAX), w)


def runs(n, omega, count, cap_div=5):
    """Whether the forced round (PSS_ANCHOR=1) is taken; cap_div: PSS_ANCHOR_CAP_DIV, clamped as the host clamps it."""
    cap_div = min(5, max(3, int(cap_div)))
    return omega >= 2 and n >= MIN_N and count <= n // cap_div


def depth_of(st):
    """The depth at which a build asks for the anchor round: the symbols of its initial key (one less when the key leaves
    out low bits of its last symbol) and what its text rounds added.  anchor_depth says the same when the round ran."""
    b = int(st['code_bits'])
    h0 = int(st['key_chars']) - (1 if int(st['key_bits']) < int(st['key_chars']) * b else 0)
    return h0 + min(16, 64 // b) * int(st['text_rounds'])


# ---- the texts -------------------------------------------------------------------------------------------------------

def _gram(alpha, length):
    g = 2
    while alpha ** g < 4 * length * length:
        g += 1
    return g


def _word(rng, symbols, length):
    """A random word all of whose windows of _gram() symbols are different: no period, no repeat inside it."""
    a = np.frombuffer(bytes(symbols), dtype=np.uint8)
    g = _gram(len(a), length)
    while True:
        w = a[rng.integers(0, len(a), length)]
        if len({bytes(w[i:i + g]) for i in range(length - g + 1)}) == length - g + 1:
            return w


def _planted(rng, n, symbols, block, starts):
    """n - 1 bytes of uniform fill with `block` at the given starts, and the newline."""
    a = np.frombuffer(bytes(symbols), dtype=np.uint8)
    t = a[rng.integers(0, len(a), n)]
    L = len(block)
    starts = sorted(int(s) for s in starts)
    for s0, s1 in zip(starts, starts[1:]):
        assert s0 + L < s1, (starts, L)                            # fresh fill between two copies
    assert starts[0] >= 0 and starts[-1] + L <= n - 1
    for s in starts:
        t[s:s + L] = block
    t[n - 1] = NL
    return t


def check_copies(t, block, starts, offsets=None):
    """The construction: a newline at the end, the block at exactly these places (overlapping occurrences would count),
    the same for the block's own suffixes, gaps of differing lengths, and neither long runs nor one word over and over."""
    t = np.ascontiguousarray(t)
    L = len(block)
    starts = sorted(int(s) for s in starts)
    assert t[-1] == NL
    for s in starts:
        assert np.array_equal(t[s:s + L], block)
    blk = bytes(block)
    assert count_sharing(t, blk) == len(starts)
    for off in (offsets if offsets is not None else (1, L // 3, (2 * L) // 3)):
        assert count_sharing(t, blk[off:]) == len(starts), off
    gaps = [starts[0]] + [b - a - L for a, b in zip(starts, starts[1:])]
    assert len(set(gaps)) == len(gaps) and min(gaps[1:]) >= 1, gaps
    assert (1 + int(np.count_nonzero(t[1:] != t[:-1]))) * 8 > t.size
    _check_not_periodic(t)


def _check_not_periodic(t):
    """A text with a period p repeats its head at p: short texts are tried at every p, longer ones show it by a head of 40
    bytes that occurs once."""
    x = t[:t.size - 1]
    if x.size <= 256:
        assert not any(np.array_equal(x[p:], x[:x.size - p]) for p in range(1, x.size // 2 + 1))
    else:
        assert count_sharing(x, bytes(x[:40])) == 1


def tiled_starts(n, L):
    """Where the copies of tiled() lie: one early, one across the border of the first tile when the text goes on behind
    it, one more inside the second tile when there is room, and one that ends with the last byte before the newline."""
    last = n - 1 - L
    if n <= 66:
        return [5, last]
    starts = [137]
    across = ANC_TILE - L // 2
    if across + L + 3 < last:
        starts.append(across)
        mid = across + L + 211
        if mid + L + 7 < last:
            starts.append(mid)
    elif 137 + L + 29 + L + 5 < last:
        starts.append(137 + L + 29)
    starts.append(last)
    return starts


def tiled(n, alpha, seed=0):
    """See the module's docstring.  n = 63 .. 65: two copies of 24 bytes; otherwise copies of 304 bytes."""
    symbols = ALPHABETS[alpha]
    tiny = n <= 66
    L = 24 if tiny else 304
    for attempt in range(64):
        rng = np.random.default_rng([n, alpha, seed, attempt])
        block = _word(rng, symbols, L)
        starts = tiled_starts(n, L)
        t = _planted(rng, n, symbols, block, starts)
        if alpha == 256 and not tiny and np.unique(t).size != 256:
            continue                                               # (the raw-byte branch wants every byte value, 0 included)
        try:
            check_copies(t, block, starts, offsets=(1,) if tiny else None)
        except AssertionError:
            if tiny:
                continue                                           # (24 bytes over two letters: a chance repeat in the fill)
            raise
        break
    else:
        raise AssertionError(('tiled', n, alpha))
    check_tiled(t, n, alpha, L, starts)
    return t


def copies_of_tiled(n):
    L = 24 if n <= 66 else 304
    return L, tiled_starts(n, L)


def check_tiled(t, n, alpha, L, starts):
    assert t.size == n and t[-1] == NL
    assert starts[-1] + L == n - 1                                  # the last copy ends with the text
    covered = np.zeros(n, bool)
    for s in starts:
        covered[s:s + L] = True
    assert covered[max(0, n - 17):n - 1].all()                      # the last 16 positions and the partial uint4 lie inside a copy
    if n - 1 > ANC_TILE:
        # the last 16 window starts of the first tile and the first ones of the second, inside one copy
        assert any(s <= ANC_TILE - 16 and s + L >= min(ANC_TILE + 16, n - 1) for s in starts), starts
    if alpha == 256 and n >= 4095:
        assert np.unique(t).size == 256 and (t == 0).any()
        assert np.array_equal(codes_of(t), t)
    else:
        assert int(codes_of(t).max()) == np.unique(t).size <= len(ALPHABETS[alpha]) + 1


# ---- ladder ----------------------------------------------------------------------------------------------------------

LADDER = ((24, 200), (40, 300), (56, 200), (72, 40), (88, 10), (320, 2))      # (length of the word, copies)
LADDER_N = 60001


def ladder():
    """Two letters and the newline (2-bit codes): words of LADDER's lengths, each written as often as LADDER says, in random
    order with fresh fill of random lengths between them.  check_ladder() holds the drain condition on the suffix array."""
    rng = np.random.default_rng(71)
    symbols = ALPHABETS[2]
    units = []
    for length, copies in LADDER:
        units += [_word(rng, symbols, length)] * copies
    units = [units[i] for i in rng.permutation(len(units))]
    a = np.frombuffer(symbols, dtype=np.uint8)
    n = LADDER_N
    t = a[rng.integers(0, 2, n)]
    room = n - 1 - sum(len(u) for u in units)
    gaps = 1 + rng.multinomial(room - len(units) - 1, np.full(len(units) + 1, 1.0 / (len(units) + 1)))
    at = 0
    for u, g in zip(units, gaps[:-1]):
        at += int(g)
        t[at:at + len(u)] = u
        at += len(u)
    assert at + int(gaps[-1]) == n - 1
    t[n - 1] = NL
    assert np.unique(t).size == 3                                   # 2-bit codes: a text round adds 16 symbols
    assert (1 + int(np.count_nonzero(t[1:] != t[:-1]))) * 8 > n
    return t


def tied_at(t, sa, depths, cap=128):
    """Number of suffixes that share at least h symbols with a neighbour in the suffix array, for every h of `depths`:
    what a round at depth h has on its active list."""
    t = np.ascontiguousarray(t)
    sa = np.asarray(sa, dtype=np.int64)
    n = t.size
    assert max(depths) <= cap
    a, b = sa[:-1], sa[1:]
    lcp = np.zeros(n - 1, np.int64)
    alive = np.ones(n - 1, bool)
    for k in range(cap):                       # (neighbour LCPs, capped: no depth asked for lies beyond)
        alive = alive & (a + k < n) & (b + k < n) & (t[np.minimum(a + k, n - 1)] == t[np.minimum(b + k, n - 1)])
        lcp += alive
    out = []
    for h in depths:
        near = np.zeros(n, bool)
        near[:-1] |= lcp >= h
        near[1:] |= lcp >= h
        out.append(int(near.sum()))
    return out


def check_ladder(t, sa):
    """The drain condition of Rounds::text_round (m * 10 <= m_prev * 6 before every text round after the first) from the key's
    16 symbols -- or 15, should the key leave out bits of its last one -- to a depth of at least 79, and ties left there:
    the window is then 64 wide whether or not the fifth round runs.  Returns the counts."""
    out = {}
    for h0 in (16, 15):
        m = tied_at(t, sa, [h0 + 16 * r for r in range(6)])
        for r in (0, 1, 2):                  # before the second, third and fourth round (the first always runs)
            assert m[r + 1] * 10 <= m[r] * 6, (h0, r, m)
        assert m[4] > 0 and m[5] > 0, (h0, m)
        assert window_of(h0 + 64) == Window(64, 8)
        out[h0] = m
    return out


# ---- on the cap ------------------------------------------------------------------------------------------------------

CAP_N = 40001
CAP_MIN = 2 * ANC_TILE
CAP_W = 8                 # 3-bit codes: 16 symbols in the initial key (or 15) and one text round of 16, a depth of >= 28


def cap_base(seed=9):
    """A text whose prefixes on_the_cap() scans: tiled(), 40 001 bytes over 4 symbols."""
    return tiled(CAP_N, 4, seed=seed)


def cap_block(t):
    """The block of a prefix of cap_base(): its first copy."""
    L, starts = copies_of_tiled(CAP_N)
    return t[starts[0]:starts[0] + L]


def _prefix(base, n):
    t = base[:n].copy()
    t[n - 1] = NL
    return t


def _cap_counts(base, omega, w, lo, hi):
    """anchor_count of every prefix base[:n - 1] + newline, lo <= n < hi, from ONE pass over the base: the windows that end
    before the last w bytes of a prefix choose what they choose in the base; only the last omega + w windows are redone."""
    codes = codes_of(base)
    nl = int(codes[-1])
    assert nl == 1 and np.array_equal(np.unique(base[:lo - 1]), np.unique(base[:-1]))      # the same codes in every prefix
    hf = [int(v) for v in hashes(codes, w)]
    mf = choices(codes, omega, w)
    upto = np.concatenate([[1], 1 + np.cumsum(mf[1:] != mf[:-1])])      # anchors chosen by the windows 0 .. s of the base
    mf = [int(v) for v in mf]
    cl = [int(v) for v in codes]
    mask = (1 << 64) - 1
    for n in range(hi - 1, lo - 1, -1):
        s0 = n - w - omega
        h = hf[s0:n - w]
        for p in range(n - w, n):
            x = 0
            for j in range(w):
                q = p + j
                c = cl[q] if q < n - 1 else (nl if q == n - 1 else 0)
                x |= c << (8 * j)
            h.append(((x * ANC_MULT) & mask) >> 33)
        h += [ANC_HMAX] * omega
        cnt = int(upto[s0])
        prev = mf[s0]
        for s in range(s0 + 1, n):
            win = h[s - s0:s - s0 + omega]
            m = s + win.index(min(win))
            cnt += m != prev
            prev = m
        yield n, cnt


_CAP = {}


def on_the_cap(div, w=8):
    """(omega, the prefix with anchor_count == n // div, the prefix with anchor_count == n // div + 1) for hashes of w bytes.
    Both prefixes are longer than two tiles, so the early copy, the one across the first tile border and the one behind it
    are whole in them."""
    key = (div, w)
    if key not in _CAP:
        # (the first text and window that have both lengths: the count walks around n / div, it need not touch it)
        for base, omega in ((cap_base(seed), omega) for seed in range(9, 15) for omega in CAP_OMEGAS[div]):
            on, over = [], []
            for n, cnt in _cap_counts(base, omega, w, CAP_MIN, CAP_N):      # (longest first, until both are found)
                if cnt == n // div and not on:
                    on.append(n)
                if cnt == n // div + 1 and not over:
                    over.append(n)
                if on and over:
                    break
            if on and over:
                break
        else:
            raise AssertionError(('no prefix on the cap', div, w))
        a, b = _prefix(base, on[0]), _prefix(base, over[0])
        for t, want in ((a, a.size // div), (b, b.size // div + 1)):
            assert anchor_count(codes_of(t), omega, w) == want      # (the model proper, on the prefix itself)
        a.setflags(write=False)
        b.setflags(write=False)
        _CAP[key] = (omega, a, b)
    return _CAP[key]


# ---- deep ------------------------------------------------------------------------------------------------------------

DEEP_N = 1 << 18


def _deep(n, alpha, seed):
    symbols = ALPHABETS[alpha]
    rng = np.random.default_rng([n, alpha, seed, 5])
    a = np.frombuffer(bytes(symbols), dtype=np.uint8)
    L = n // 8
    block = a[rng.integers(0, len(a), L)]
    k = 5
    room = n - 1 - k * L
    gaps = 1 + rng.multinomial(room - (k + 1), np.full(k + 1, 1.0 / (k + 1)))
    starts = []
    at = 0
    for g in gaps[:-1]:
        at += int(g)
        starts.append(at)
        at += L
    return _planted(rng, n, symbols, block, starts), block, starts


def deep(n, alpha, seed=0):
    """Five copies of one random block of n / 8 bytes, fresh fill of random lengths between them."""
    t, block, starts = _deep(n, alpha, seed)
    _check_deep(t, block, starts)
    return t


def copies_of_deep(n, alpha, seed=0):
    _, block, starts = _deep(n, alpha, seed)
    return len(block), starts


def _check_deep(t, block, starts):
    L = len(block)
    assert t[-1] == NL
    for s in starts:
        assert np.array_equal(t[s:s + L], block)
    assert count_sharing(t, bytes(block[:48])) == len(starts) and count_sharing(t, bytes(block[L - 48:])) == len(starts)
    gaps = [starts[0]] + [b - a - L for a, b in zip(starts, starts[1:])]
    assert len(set(gaps)) == len(gaps) and min(gaps[1:]) >= 1
    assert (1 + int(np.count_nonzero(t[1:] != t[:-1]))) * 8 > t.size
    _check_not_periodic(t)
