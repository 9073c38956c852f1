"""Texts that put the two partition passes of the MSD sort (msd_sort.hip) on the edges of their 16384-element tiles, and
the numpy model whose asserts say that the texts hold those edges.  Everything here runs on the CPU;
tests/test_scatter_tile_texts.py runs every generator, tests/test_scatter_tiles_gpu.py sorts the texts on the GPU.

First pass (msd_scatter2_kernel from the text): range r covers tiles_per_range1 * 8192 suffixes, walked in tiles of 16384;
thread tid of a tile packs the keys of the sixteen suffixes from i0 = tile start + 16 tid and asks for the code words of its
next tile while the current one is written out.  A range of one tile never carries words ahead, a range of a tile and a
half carries them into a tile whose upper half no thread stages, and the guard "i0 < n" decides near the text's end.

Second pass in LSD order (msd_scatter_lb_kernel): every d-region -- the suffixes that share the SECOND ten bits of their
joint bucket number -- is cut into tiles of 16384, the last one short.  The P2 case plants symbols until six regions
have sizes of 0, 1, 8191, 8192, 8193 and 16383 mod 16384 (the search is seeded).

The texts are random lines over the 39 symbols of bench.py's `lines` corpus (38 + the newline): 6-bit codes."""
import numpy as np

from tests import sa_edge_texts as E

ALPHA = b'abcdefghijklmnopqrstuvwxyz0123456789 .'      # bench.py's ALPHA
SYMS = np.frombuffer(bytes(sorted(ALPHA + b'\n')), dtype=np.uint8)      # byte order = code order: code of SYMS[i] is i + 1
B = 6                                                  # code bits of 39 symbols
TILE = 8192                                            # MSD_TILE: the unit of the first pass's ranges
TILE2 = 16384                                          # MSD_TILE2: the tile of both passes
G1_RANGES = 1024
BLOCK = 1024
IPT = TILE2 // BLOCK                                   # 16 suffixes per thread
RESIDUES = (0, 1, 8191, 8192, 8193, 16383)


def lines(n, seed):
    """n bytes of random lines (20 .. 100 symbols and a newline) over ALPHA, the last byte a newline."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(ALPHA, dtype=np.uint8)
    t = a[rng.integers(0, len(a), n)]
    ends = np.cumsum(rng.integers(21, 102, n // 21 + 2)) - 1
    t[ends[ends < n]] = E.NL
    t[n - 1] = E.NL
    return t


def codes_of(t):
    """Dense codes 1 .. 39 in byte order, three zeros behind the text."""
    present = np.flatnonzero(np.bincount(t, minlength=256))
    assert present.size == SYMS.size and (present == SYMS).all(), present.size
    lut = np.zeros(256, np.uint32)
    lut[SYMS] = np.arange(1, SYMS.size + 1, dtype=np.uint32)
    return np.concatenate([lut[t], np.zeros(3, np.uint32)])


def joint(t):
    """Joint bucket number of every suffix: the top 20 bits of its key = three 6-bit codes and the top two bits of a fourth."""
    c = codes_of(t)
    n = t.size
    return (c[:n] << 14) | (c[1:n + 1] << 8) | (c[2:n + 2] << 2) | (c[3:n + 3] >> 4)


def region_sizes(t):
    """Suffixes per d-region: d = the low ten bits of the joint bucket number (the first pass's digit in LSD order)."""
    return np.bincount(joint(t) & 1023, minlength=1024)


class Geometry:
    """The first pass's ranges and tiles for a text of n bytes, as msd_suffix_sort lays them out."""

    def __init__(self, n):
        self.n = n
        tiles = (n + TILE - 1) // TILE
        self.tiles_per_range1 = (tiles + G1_RANGES - 1) // G1_RANGES
        self.num_ranges1 = (tiles + self.tiles_per_range1 - 1) // self.tiles_per_range1
        span = self.tiles_per_range1 * TILE
        self.e0 = np.arange(self.num_ranges1, dtype=np.int64) * span
        self.e1 = np.minimum(self.e0 + span, n)
        assert (self.e0 < self.e1).all() and self.e1[-1] == n

    def tiles_of(self, r):
        """(base, valid) of the tiles of range r."""
        return [(int(b), int(min(TILE2, self.e1[r] - b))) for b in range(int(self.e0[r]), int(self.e1[r]), TILE2)]

    def ahead_carries(self):
        """Is there a tile behind which its range goes on (the loads ahead carry words)?"""
        return self.tiles_per_range1 * TILE > TILE2 and int((self.e1 - self.e0).max()) > TILE2

    def last_tile_threads(self):
        """i0 of every thread of the text's last tile."""
        base, _ = self.tiles_of(self.num_ranges1 - 1)[-1]
        return base + np.arange(BLOCK, dtype=np.int64) * IPT


def check_text(t, tiles_per_range1=None):
    """What every case must hold: the 39 symbols, no joint bucket beyond a local-sort tile, the expected range length."""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    assert t[-1] == E.NL
    j = joint(t)
    assert int(np.bincount(j, minlength=1 << 20).max()) <= E.MSD_MAX_BUCKET
    g = Geometry(t.size)
    if tiles_per_range1 is not None:
        assert g.tiles_per_range1 == tiles_per_range1, (g.tiles_per_range1, tiles_per_range1)
    return g


# ---- steering region sizes -----------------------------------------------------------------------------------------

def _digit_parts(d):
    """The codes a d-region asks of the three symbols behind a suffix's first: (low two bits of the second symbol's
    code, the third symbol's code, top two bits of the fourth's)."""
    return d >> 8, (d >> 2) & 63, d & 3


def steer(t, seed, want):
    """Rewrites symbols of t (in place) until region d holds want[d] mod 16384 suffixes, for every d of `want`.  To grow a
    region, three symbols with the region's digit are written at random places (the symbol before them, the second
    symbol's high bits and the fourth's low bits are left to chance: no joint bucket grows with the region); to shrink it,
    the third symbol of random members is replaced.  Every edit moves a few suffixes between other regions as well, so
    the sizes are counted anew and the rest is done again: the error shrinks by an order of magnitude per round."""
    rng = np.random.default_rng(seed)
    n = t.size
    code = np.arange(2, SYMS.size + 1)                       # codes of the symbols of ALPHA (code 1 is the newline)
    for _ in range(40):
        dv = joint(t) & 1023
        size = np.bincount(dv, minlength=1024)
        todo = {}
        for d, r in want.items():
            up = (r - int(size[d])) % TILE2
            todo[d] = up if up <= TILE2 // 2 or int(size[d]) - (TILE2 - up) < 0 else up - TILE2
        if not any(todo.values()):
            return
        for d, m in todo.items():
            lo2, c3, hi2 = _digit_parts(d)
            if m > 0:
                at = rng.integers(8, n - 8, m)
                t[at + 1] = SYMS[rng.choice(code[(code & 3) == lo2], m) - 1]
                t[at + 2] = SYMS[c3 - 1]
                t[at + 3] = SYMS[rng.choice(code[(code >> 4) == hi2], m) - 1]
            elif m < 0:
                members = np.flatnonzero(dv[8:n - 8] == d) + 8
                at = rng.choice(members, -m, replace=False)
                t[at + 2] = SYMS[rng.choice(code[code != c3], -m) - 1]
    raise AssertionError('the region sizes did not settle')


def pick_regions(t, seed, k):
    """k d-regions to steer: non-empty ones whose digit can be written with symbols of ALPHA (the third symbol's code is
    one of 2 .. 39, the fourth's top two bits are not 3)."""
    size = region_sizes(t)
    d = np.arange(1024)
    c3 = (d >> 2) & 63
    cand = d[(size > 0) & (c3 >= 2) & (c3 <= SYMS.size) & ((d & 3) < 3)]
    return [int(x) for x in np.random.default_rng(seed).choice(cand, k, replace=False)]


# ---- the cases -------------------------------------------------------------------------------------------------------

def short_case(n):
    """One short tile: the upper half of the staging area is never written, nothing is loaded ahead."""
    t = lines(n, 9100 + n % 97)
    g = check_text(t, 1)
    assert g.num_ranges1 == -(-n // TILE) and not g.ahead_carries()
    assert all(len(g.tiles_of(r)) == 1 for r in range(g.num_ranges1))
    assert (joint(t) == E.joint_buckets(t, B)).all()         # both digits as the model of the other tests has them
    return t


def full_case():
    """Every range is exactly one full tile of 16384 with nothing behind it -- and the regions of the second pass sit on
    every edge of ITS tiles: sizes of 0, 1, 8191, 8192, 8193 and 16383 mod 16384, and an empty region."""
    n = (1 << 23) + 2 * TILE
    t = lines(n, 9201)
    regions = pick_regions(t, 9202, len(RESIDUES))
    want = dict(zip(regions, RESIDUES))
    steer(t, 9203, want)
    g = check_text(t, 2)
    assert not g.ahead_carries() and all(g.tiles_of(r) == [(int(g.e0[r]), TILE2)] for r in range(g.num_ranges1))
    size = region_sizes(t)
    for d, r in want.items():
        assert size[d] > 0 and size[d] % TILE2 == r, (d, int(size[d]), r)
    assert {int(s) % TILE2 for s in size[size > 0]} >= set(RESIDUES)
    assert int(np.count_nonzero(size == 0)) >= 1
    return t


HALF_DS = (1, 7, 16, 8191)


def half_case(d):
    """A full tile, then a half tile: the words loaded ahead belong to a tile of 8192; the text ends d elements into the
    last range's second tile."""
    n = (1 << 24) + 3 * TILE + d
    t = lines(n, 9300 + d)
    g = check_text(t, 3)
    assert g.ahead_carries()
    assert g.tiles_of(0) == [(0, TILE2), (TILE2, TILE)]
    last = g.tiles_of(g.num_ranges1 - 1)
    assert len(last) == 2 and last[0][1] == TILE2 and last[1][1] == d, last
    _guards(g)
    return t


def several_case():
    """Ranges of two full tiles (every range carries words ahead once and stops), the last range short."""
    n = 3 * (1 << 23) + TILE + 5
    t = lines(n, 9401)
    g = check_text(t, 4)
    assert g.ahead_carries() and g.tiles_of(0) == [(0, TILE2), (TILE2, TILE2)]
    assert g.tiles_of(g.num_ranges1 - 1) == [(int(g.e0[-1]), TILE + 5)]
    _guards(g)
    return t


def _guards(g):
    """The text ends inside a thread's sixteen suffixes, and behind it the same tile has threads with nothing to load."""
    i0 = g.last_tile_threads()
    assert ((i0 < g.n) & (g.n <= i0 + IPT)).any()
    assert (i0 >= g.n).any()


CASES = {'short5000': lambda: short_case(5000), 'short8193': lambda: short_case(TILE + 1), 'full': full_case,
         **{f'half{d}': (lambda d=d: half_case(d)) for d in HALF_DS}, 'several': several_case}
