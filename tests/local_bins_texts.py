"""Texts that put msd_local_fast_kernel (msd_sort.hip) on the edges of its BINS -- 8192 of them, the top 13 bits of a
tile's local key, counted in one array of 16-bit counters whose entries end up as the bins' ends (the start of bin b is
read from entry b - 1, a zero halfword in front serves bin 0); a ranking window of LS_WINDOW members; a tile declined
when more than LS_KMAX elements share the top 12 bits, that is the pair of bins b & ~1, b | 1 -- and the numpy
restatement the GPU tests compare with (tests/test_local_bins_gpu.py).  Everything here runs on the CPU;
tests/test_local_bins_texts.py runs every generator.

The construction is that of tests/local_rows_texts.py (heads lead + S1 + S2 + three continuation symbols over FILL70,
7-bit codes, a lead byte = a tile of its own): below the bucket lie 22 key bits [s2 & 1 | c1 | c2 | c3], so the bin of an
element of a one-bucket tile is [s2 & 1 | code(c1) | code(c2) >> 2] and its pair [s2 & 1 | code(c1) | code(c2) >> 3].
Plan restates the tile plan and the local key for any key format and both digit orders; every generator asserts the
geometry it is about (which bin, how many members, which positions) and the tiles the model expects to be declined."""
import numpy as np

from tests import msd_finish_texts as F
from tests import sa_edge_texts as E
from tests.local_rows_texts import LEADS, S1, S2, View, _cont_bytes, assemble, conts

ROW = 512
BIN_BITS = 13                                # LS_BIN_BITS
DECLINE_BITS = 12                            # LS_DECLINE_BITS
LS_WINDOW = 7
A = len(E.FILL70)
S2_ODD = E.FILL70[21]                        # code 23: the same joint bucket as S2 (code 22), s2 & 1 = 1
PITCH = 16


class Plan:
    """The tiles of a text under a key format (PSS_MSD_KEY_CAP = cap, PSS_MSD_PARTIAL_SYMBOL = partial) and a digit order,
    and the local key of every element: [bucket inside the tile | the rem = key_bits - 20 key bits below the bucket] --
    the bucket inside the tile being the difference of the buckets' tags (LSD order: the LSD number mod 64, a tile spans
    nb = last - first + 1 of them; MSD order: the number among the non-empty buckets, nb = the tile's buckets)."""

    def __init__(self, t, lsd=True, **fmt):
        t = np.ascontiguousarray(t, dtype=np.uint8)
        self.t, self.n, self.lsd = t, t.size, lsd
        self.f = f = F.Format(t.size, int(np.unique(t).size), lsd=lsd, **fmt)
        self.rem = rem = f.kb - 20
        key = F._pack(F.codes_of(t), t.size, 0, f.kc, f.b) >> np.uint64(f.drop)
        self.order = np.lexsort((np.arange(t.size), key))
        self.keys = key[self.order]
        numbers, sizes = np.unique(self.keys >> np.uint64(rem), return_counts=True)
        n2, s2 = E.bucket_sizes(t)
        assert np.array_equal(numbers.astype(np.int64), n2) and np.array_equal(sizes, s2)
        self.numbers, self.sizes = n2, sizes
        self.head = head = E.tile_heads(n2, sizes, t.size, lsd)
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        first = np.flatnonzero(head)
        last = np.append(first[1:], len(sizes)) - 1
        self.e0 = start[:-1][first]
        self.counts = np.diff(np.append(self.e0, t.size))
        self.buckets = last - first + 1                                   # non-empty buckets per tile
        tag = (E.lsd_numbers(n2) & (E.MSD_RAW_TAG_SPAN - 1)) if lsd else np.arange(len(sizes))
        self.nb = tag[last] - tag[first] + 1
        assert (self.nb >= 1).all() and (self.nb <= (E.MSD_RAW_TAG_SPAN if lsd else E.MSD_TAG_SPAN)).all()
        self.seg = np.array([int(x - 1).bit_length() for x in self.nb])
        tile_of_bucket = np.cumsum(head) - 1
        self.rel = (tag - tag[first][tile_of_bucket]).astype(np.uint64)
        self.tile = np.repeat(tile_of_bucket, sizes)
        self.local = (np.repeat(self.rel, sizes) << np.uint64(rem)) | (self.keys & np.uint64((1 << rem) - 1))

    def sort_bits(self, i):
        return self.rem + int(self.seg[i])

    def bins(self, i, bits=BIN_BITS):
        """Bin of every position of tile i (positions in key order: the bins only grow)."""
        e0, c = int(self.e0[i]), int(self.counts[i])
        return (self.local[e0:e0 + c] >> np.uint64(max(0, self.sort_bits(i) - bits))).astype(np.int64)

    def bin_table(self, i, bits=BIN_BITS):
        """(bin numbers, sizes, first positions) of the populated bins of tile i."""
        v, first, cnt = np.unique(self.bins(i, bits), return_index=True, return_counts=True)
        return v, cnt, first

    def slow_tiles(self):
        """Tiles with more than LS_KMAX elements under one value of the top DECLINE_BITS bits of the local key."""
        out = []
        for i in range(len(self.e0)):
            if int(self.counts[i]) > E.LS_KMAX and int(self.bin_table(i, DECLINE_BITS)[1].max()) > E.LS_KMAX:
                out.append(i)
        return out

    def tile_of_lead(self, lead):
        """The tile that holds the suffixes starting with this byte -- which must be all of it."""
        slots = np.flatnonzero(self.t[self.order] == lead)
        i = int(np.searchsorted(self.e0, slots[0], side='right')) - 1
        assert slots[0] == self.e0[i] and slots.size == self.counts[i] and slots[-1] == self.e0[i] + slots.size - 1, lead
        return i


def _cells(c1, lo, hi):
    """Continuation numbers with first symbol FILL70[c1] and a second symbol of code lo .. hi - 1 (code = index + 2)."""
    return np.array([c1 * A * A + (code - 2) * A + c for code in range(lo, hi) for c in range(A)])


def _draw(rng, pool, k):
    return [int(v) for v in rng.choice(pool, size=k, replace=False)]


def pair_conts(rng, k, lower, upper, c1=A - 1):
    """k continuations without ties; the largest lower + upper of them share a 12-bit bin (first symbol FILL70[c1], second
    symbol of code 8 .. 15), `lower` in its lower half (codes 8 .. 11) and `upper` in its upper half (12 .. 15); the
    others start with one of the symbols below FILL70[A - 3]."""
    big = _draw(rng, _cells(c1, 8, 12), lower) + _draw(rng, _cells(c1, 12, 16), upper)
    return sorted(_draw(rng, np.arange(0, (A - 3) * A * A), k - lower - upper) + big)


def edge_conts(rng, k, m, below, c1=35):
    """k continuations without ties: m in ONE bin (first symbol FILL70[c1], second symbol of code 8 .. 11), `below` of them
    with a smaller first symbol and the rest with a larger one -- the bin takes positions below .. below + m - 1."""
    return sorted(_draw(rng, np.arange(0, c1 * A * A), below) + _draw(rng, _cells(c1, 8, 12), m) +
                  _draw(rng, np.arange((c1 + 1) * A * A, A ** 3), k - m - below))


def _one_bucket_bin(c1_code, c2_code, odd=False):
    return (int(odd) << 12) | (c1_code << 5) | (c2_code >> 2)


def _check_default(t, expect_slow_leads):
    """The model of local_rows_texts and the one of this file agree on the tiles to decline: those of the given leads."""
    v, p = View(t), Plan(t)
    assert p.rem == 22 and np.array_equal(v.e0, p.e0)
    want = sorted(p.tile_of_lead(lead) for lead in expect_slow_leads)
    assert v.slow_tiles() == want and p.slow_tiles() == want, (v.slow_tiles(), p.slow_tiles(), want)
    return p


# ---- split pairs -----------------------------------------------------------------------------------------------------

KEEP_SPLITS = ((32, 32), (0, 64), (64, 0))
DECLINE_SPLITS = ((64, 1), (1, 64), (33, 32))


def _check_split(p, lead, k, lower, upper, c1=A - 1):
    i = p.tile_of_lead(lead)
    assert int(p.counts[i]) == k and p.buckets[i] == 1 and p.sort_bits(i) == 22
    b, cnt, first = p.bin_table(i)
    lo_bin = _one_bucket_bin(c1 + 2, 8)                                   # code(c2) >> 2 = 2 | 3
    got = {int(x): int(c) for x, c in zip(b, cnt) if x >> 1 == lo_bin >> 1}
    assert got == {bn: c for bn, c in ((lo_bin, lower), (lo_bin + 1, upper)) if c}, got
    assert int(b[-1]) >> 1 == lo_bin >> 1 and int(first[b >> 1 == lo_bin >> 1][0]) == k - lower - upper      # the tile's last elements
    assert k - lower - upper >= (k - 1) // ROW * ROW                                                     # all in the tail row
    rest = cnt[b >> 1 != lo_bin >> 1]
    assert int(rest.max()) <= LS_WINDOW                                   # no other bin leaves the window
    return i


def split_keep_case():
    """Three tiles of 600 whose last 64 elements share a 12-bit bin -- exactly LS_KMAX -- as 32 + 32, 0 + 64 and 64 + 0 over
    its two 13-bit halves: nothing is declined.  (Each tile has a first continuation symbol of its own for the 64: the
    suffixes one byte into the copies share a tile too, and bins there.)"""
    rng = np.random.default_rng(9101)
    tiles = [(LEADS[j], pair_conts(rng, 600, lo, up, A - 1 - j)) for j, (lo, up) in enumerate(KEEP_SPLITS)]
    t = assemble((1 << 17) + 19, 9102, tiles)
    p = _check_default(t, [])
    for j, ((lead, _), (lo, up)) in enumerate(zip(tiles, KEEP_SPLITS)):
        _check_split(p, lead, 600, lo, up, A - 1 - j)
    return t


def split_decline_case(lower, upper):
    """One tile of 600 whose last 65 elements share a 12-bit bin, split over its halves: the tile is declined -- with 64 + 1
    (1 + 64) the single member never sees a bin longer than the window, its 64 neighbours do."""
    assert lower + upper == E.LS_KMAX + 1
    rng = np.random.default_rng(9200 + lower)
    t = assemble((1 << 17) + 31 + lower, 9300 + lower, [(LEADS[0], pair_conts(rng, 600, lower, upper))])
    p = _check_default(t, [LEADS[0]])
    _check_split(p, LEADS[0], 600, lower, upper)
    return t


# ---- window edges, empty neighbours ----------------------------------------------------------------------------------

# (elements, members of the bin, elements before it): the bin in the tail row, in a full row, across the first row border
EDGE_TILES = tuple((k, m, below) for m in (LS_WINDOW, LS_WINDOW + 1)
                   for k, below in ((600, 600 - m), (1100, 100), (1100, 508)))
GAP_TILE = (600, 3, 300)


def edges_case():
    """Bins of LS_WINDOW and LS_WINDOW + 1 members as the last elements of a tail row, inside a full row and on positions
    508 .. 514 (515) -- across the border of rows 0 and 1 --, and a bin of three between 960 empty bins on either side (its
    start is the end of an empty bin, and so is the start of the populated bin after it)."""
    rng = np.random.default_rng(9401)
    tiles = [(LEADS[j], edge_conts(rng, k, m, below)) for j, (k, m, below) in enumerate(EDGE_TILES)]
    k, m, below = GAP_TILE
    gap = sorted(_draw(rng, np.arange(0, 5 * A * A), below) + _draw(rng, _cells(35, 8, 12), m) +
                 _draw(rng, np.arange(65 * A * A, A ** 3), k - m - below))
    tiles.append((LEADS[len(EDGE_TILES)], gap))
    t = assemble((1 << 17) + 43, 9402, tiles)
    p = _check_default(t, [])
    target = _one_bucket_bin(37, 8)
    for (lead, _), (k, m, below) in zip(tiles, EDGE_TILES + (GAP_TILE,)):
        i = p.tile_of_lead(lead)
        b, cnt, first = p.bin_table(i)
        at = int(np.flatnonzero(b == target)[0])
        assert int(p.counts[i]) == k and int(cnt[at]) == m and int(first[at]) == below, (k, m, below)
    for k, m, below in EDGE_TILES:
        rows = {below // ROW, (below + m - 1) // ROW}
        full = (k - 1) // ROW
        assert (below == 508) == (rows == {0, 1}) and (k == 600) == (rows == {full}) and (below == 100) == (rows == {0} and full > 0)
    i = p.tile_of_lead(LEADS[len(EDGE_TILES)])
    b = p.bin_table(i)[0]
    at = int(np.flatnonzero(b == target)[0])
    assert target - int(b[at - 1]) > 900 and int(b[at + 1]) - target > 900          # long runs of empty bins on both sides
    return t


# ---- first and last bin ----------------------------------------------------------------------------------------------

TOPS = (0xFC, 0xFD, 0xFE, 0xFF)              # with 127 symbols in the text: codes 124 .. 127
FILLERS = tuple(range(118, 118 + 51))        # bytes that only bring the alphabet to 127 symbols


def _assemble_raw(n, seed, copies, singles=()):
    """Random text of n bytes over FILL70 ending in a newline, the copies (byte strings of at most 8 bytes) shuffled and
    PITCH bytes apart from byte 8 on, every byte of `singles` written once near the end."""
    rng = np.random.default_rng(seed)
    t = np.empty(n, np.uint8)
    t[:n - 1] = E._fill(rng, E.FILL70, n - 1)
    t[n - 1] = E.NL
    assert all(len(c) <= 8 for c in copies) and 8 + PITCH * len(copies) < n - 8 - 4 * len(singles) - 64
    for i, j in enumerate(rng.permutation(len(copies))):
        c = copies[j]
        t[8 + PITCH * i:8 + PITCH * i + len(c)] = np.frombuffer(c, np.uint8)
    for j, s in enumerate(singles):
        t[n - 32 - 4 * j] = s
    return t


FIRST_LAST_Y = 99                            # (code 53; looked for once over the odd codes of FILL70 -- None searches again -- and checked below)


def _first_last_text(y):
    rng = np.random.default_rng(9501)
    head = bytes([LEADS[0], S1, S2_ODD])
    body = [head + _cont_bytes(v) for v in conts(rng, 595)]
    top = [head + bytes([0xFF, TOPS[j % 4], E.FILL70[3 * j]]) for j in range(5)]           # bin 8191 of a one-bucket tile
    # the first tile of the suffix array: the text's last suffix ("\n": every key bit below its bucket is zero) and the
    # suffixes that start "\n\n" + y -- 63 LSD numbers later when y is chosen right, which makes the tile's local key
    # [6 bits | 22 bits] and its bins [bucket | s3 & 1 | code(c1) >> 1]: 0 and, with c1 one of the two largest symbols, 8191
    twin = [bytes([E.NL, E.NL, y, TOPS[2 + j % 2], E.FILL70[j], E.FILL70[(7 * j) % A]]) for j in range(40)]
    return _assemble_raw((1 << 17) + 57, 9502, body + top + twin, FILLERS)


def first_last_case():
    """127 symbols (7-bit codes up to 127).  Tile 0 holds nothing but bin 0 (one element, the tile's smallest: the text's
    last suffix) and bin 8191 (40 elements that end at the tile's last slot: behind them the window reads the sentinels);
    the tile of LEADS[0] -- one bucket, 600 elements -- has its last five elements in bin 8191 and none in bin 0."""
    global FIRST_LAST_Y
    cands = [FIRST_LAST_Y] if FIRST_LAST_Y is not None else [c for c in E.FILL70 if (c - 48 + 2) % 2 == 1]
    for y in cands:
        t = _first_last_text(y)
        p = Plan(t)
        if int(p.nb[0]) == 64 and int(p.counts[0]) == 41:
            FIRST_LAST_Y = y
            break
    else:
        raise AssertionError('no second symbol puts the bucket 63 LSD numbers behind the first')
    assert int(np.unique(t).size) == 127 and p.f.b == 7 and p.rem == 22
    assert p.buckets[0] == 2 and p.sort_bits(0) == 28
    b, cnt, first = p.bin_table(0)
    assert b.tolist() == [0, (1 << BIN_BITS) - 1] and cnt.tolist() == [1, 40] and first.tolist() == [0, 1]
    assert p.order[0] == t.size - 1                                       # bin 0: the last suffix
    i = p.tile_of_lead(LEADS[0])
    b, cnt, first = p.bin_table(i)
    assert int(p.counts[i]) == 600 and p.sort_bits(i) == 22
    assert int(b[-1]) == (1 << BIN_BITS) - 1 and int(cnt[-1]) == 5 and int(first[-1]) == 595 and int(b[0]) >= 1 << 12
    _check_default(t, [])
    return t


# ---- key widths around the bin width ---------------------------------------------------------------------------------

WIDTH_CAPS = (30, 31, 32, 33, 34)            # PSS_MSD_KEY_CAP with PSS_MSD_PARTIAL_SYMBOL=1: 10 .. 14 key bits below the bucket
WIDTH_TILES = ((700,), (400, 400), (300, 300, 300))


def widths_text():
    """Tiles of one, two and three adjacent buckets (leads with S2, S2 + 2, S2 + 4: tags 11, 12, 13 of one block), all of a
    lead's buckets starting inside one MSD_WIN window."""
    rng = np.random.default_rng(9601)
    copies = []
    for j, sizes in enumerate(WIDTH_TILES):
        for q, k in enumerate(sizes):
            head = bytes([LEADS[j], S1, E.FILL70[20 + 2 * q]])
            copies += [head + _cont_bytes(v) for v in conts(rng, k)]
    total = len(copies)
    n = E.MSD_WIN * 21 + 100 + total                                      # the leads' first bucket starts 100 slots into a window
    return _assemble_raw(n, 9602, copies)


def widths_case(cap, lsd=True):
    """(text, plan under the format): the three tiles sort on rem, rem + 1 and rem + 2 bits, rem = cap - 20 -- over the
    five caps every number of buckets meets 12, 13 and 14 bits."""
    t = widths_text()
    p = Plan(t, lsd=lsd, cap=cap, partial=True)
    assert p.f.kb == cap and p.rem == cap - 20
    if lsd:
        for j, sizes in enumerate(WIDTH_TILES):
            i = p.tile_of_lead(LEADS[j])
            assert int(p.buckets[i]) == len(sizes) == int(p.nb[i]) and p.sort_bits(i) == cap - 20 + (0, 1, 2)[j]
            assert int(p.counts[i]) == sum(sizes)
    return t, p


def widths_cover():
    got = {j: set() for j in range(3)}
    for cap in WIDTH_CAPS:
        for j in range(3):
            got[j].add(cap - 20 + j)
    assert all({12, 13, 14} <= s for s in got.values())


# ---- counters at their ceiling ---------------------------------------------------------------------------------------

def ceiling_case():
    """The `cap` text of local_rows_texts: a tile of MSD_TILE_CAP = 8176 elements in two buckets of 4088.  The last populated
    bin is not the last bin, so every counter behind it -- upper halves of packed words included -- ends at 8176."""
    from tests.local_rows_texts import cap_case
    t = cap_case()
    p = _check_default(t, [])
    i = len(p.e0) - 1
    assert int(p.counts[i]) == E.MSD_TILE_CAP and p.buckets[i] == 2 and p.sort_bits(i) == 23
    b = p.bin_table(i)[0]
    assert int(b[-1]) < (1 << BIN_BITS) - 2 and int(b[-1]) >= 1 << 12
    return t


TEXTS = {'split_keep': split_keep_case, 'edges': edges_case, 'first_last': first_last_case, 'ceiling': ceiling_case}
TEXTS.update({'split_%d_%d' % s: (lambda s=s: split_decline_case(*s)) for s in DECLINE_SPLITS})
SLOW_TILES = {'split_keep': 0, 'edges': 0, 'first_last': 0, 'ceiling': 0}
SLOW_TILES.update({'split_%d_%d' % s: 1 for s in DECLINE_SPLITS})
