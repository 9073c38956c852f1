"""Texts that put msd_local_fast_kernel (msd_sort.hip) on the edges of its row structure -- rows of 512 positions, every
row of a tile full but the last -- and the numpy restatement the GPU tests compare with (tests/test_local_rows_gpu.py).
Everything here runs on the CPU; tests/test_local_rows_texts.py runs every generator.

The texts are random over the 70 symbols of sa_edge_texts.FILL70 with short heads planted in them.  A head is a lead byte
that occurs nowhere else, two fixed symbols and a continuation of three symbols: with 7-bit codes the sort key is exactly
those six symbols (42 bits), the joint bucket is [lead | s1 | s2 >> 1], and a lead byte of its own is a first digit of its
own -- the copies of one head are one bucket alone in its aligned block of 64 joint buckets, that is one TILE of exactly
as many elements as there are copies.  Inside the tile the order is the continuations' order, so a case chooses the sorted
position of every tie (two copies with one continuation) and the members of every bin (the top 12 of the 22 key bits
below the bucket: s2's low bit, the first continuation symbol and the top four bits of the second)."""
import numpy as np

from tests import msd_finish_texts as F
from tests import sa_edge_texts as E

ROW = 512                                    # MSD_BLOCK: positions per row
WAVE = 64
LS_WINDOW = 8
A = len(E.FILL70)                            # 70
S1, S2 = E.FILL70[10], E.FILL70[20]
LEADS = tuple(range(0xE0, 0x100))            # bytes outside FILL70 and '\n'; byte order = tile order
PITCH = 16


def _cont_bytes(v):
    """Continuation number v (base 70, most significant symbol first) -> its three bytes."""
    return bytes([E.FILL70[v // (A * A)], E.FILL70[(v // A) % A], E.FILL70[v % A]])


def conts(rng, k, pairs=(), lo=0, hi=A ** 3, first=None, last=None):
    """k continuations in sorted order, all different except that for every i of `pairs` the sorted positions i and i + 1
    hold the same one; drawn from [lo, hi); first / last: the smallest / largest one is this number."""
    pairs = set(pairs)
    assert all(0 <= i < k - 1 and i + 1 not in pairs for i in pairs)
    distinct = k - len(pairs)
    fixed = [v for v in (first, last) if v is not None]
    a, b = (first + 1 if first is not None else lo), (last if last is not None else hi)
    pool = np.sort(np.concatenate([rng.choice(np.arange(a, b), size=distinct - len(fixed), replace=False),
                                   np.array(fixed, dtype=np.int64)]))
    assert np.unique(pool).size == distinct
    out, j = [], 0
    for pos in range(k):
        if pos - 1 in pairs:
            out.append(out[-1])
        else:
            out.append(int(pool[j]))
            j += 1
    return out


def bin_conts(rng, k, m):
    """k continuations without ties of which exactly the m largest share one bin: first symbol the alphabet's last, the
    second symbol's code in one block of eight; the others start with a smaller symbol."""
    top = (A - 1) * A * A
    # codes of FILL70 are 2 .. 71: symbols 6 .. 13 have codes 8 .. 15, one value of code >> 3
    cells = [top + s * A + c for s in range(6, 14) for c in range(A)]
    big = rng.choice(np.array(cells), size=m, replace=False)
    small = rng.choice(np.arange(0, top), size=k - m, replace=False)
    return sorted(int(v) for v in np.concatenate([small, big]))


def assemble(n, seed, tiles):
    """Random text of n bytes over FILL70 ending in a newline; tiles: list of (lead byte, [continuation numbers]) -- one
    copy of lead + S1 + S2 + continuation per number, all copies of all tiles shuffled, PITCH bytes apart."""
    rng = np.random.default_rng(seed)
    t = np.empty(n, np.uint8)
    t[:n - 1] = E._fill(rng, E.FILL70, n - 1)
    t[n - 1] = E.NL
    copies = [bytes([lead, S1, S2]) + _cont_bytes(v) for lead, vs in tiles for v in vs]
    assert 8 + PITCH * len(copies) < n - 8, (len(copies), n)
    for i, j in enumerate(rng.permutation(len(copies))):
        t[8 + PITCH * i:8 + PITCH * i + 6] = np.frombuffer(copies[j], np.uint8)
    for lead, vs in tiles:
        assert int(np.count_nonzero(t == lead)) == len(vs)
    return t


class View:
    """What the sort must make of a text: the key format, the sorted keys, the tiles of the plan."""

    def __init__(self, t, lsd=True):
        t = np.ascontiguousarray(t, dtype=np.uint8)
        self.t, self.n = t, t.size
        self.f = f = F.Format(t.size, int(np.unique(t).size), lsd=lsd)
        assert (f.b, f.kc, f.kb, f.drop) == (7, 6, 42, 0), (f.b, f.kc, f.kb, f.drop)
        self.m = F.Model(t, f)
        key = F._pack(self.m.codes, t.size, 0, f.kc, f.b)
        self.order = np.lexsort((np.arange(t.size), key))
        self.keys = key[self.order]                                   # keys in suffix-array order
        self.tie = np.r_[False, self.keys[1:] == self.keys[:-1]]      # same key as my predecessor
        numbers, sizes = E.bucket_sizes(t)
        head = E.tile_heads(numbers, sizes, t.size, lsd)
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.lsd, self.numbers, self.sizes, self.head = lsd, numbers, sizes, head
        self.e0 = start[:-1][head]
        self.counts = np.diff(np.append(self.e0, t.size))
        self.buckets = np.diff(np.append(np.flatnonzero(head), len(sizes)))      # non-empty buckets per tile
        assert len(self.e0) == E.tile_count(t, lsd)

    def slow_tiles(self):
        """Tiles the fast kernel must decline: those with a bin of more than LS_KMAX members.  The local key of an element is
        [its bucket's tag - the tag of the tile's first bucket | the 22 key bits below the bucket], the tag being the
        bucket's LSD number mod 64; of its 22 + ceil(log2(span of tags)) bits the top 12 are the bin."""
        assert self.lsd
        tag = E.lsd_numbers(self.numbers) & (E.MSD_RAW_TAG_SPAN - 1)
        first = np.flatnonzero(self.head)
        last = np.append(first[1:], len(self.sizes)) - 1
        nb = tag[last] - tag[first] + 1
        seg = np.array([int(x - 1).bit_length() for x in nb])
        tile_of_bucket = np.cumsum(self.head) - 1
        rel = (tag - tag[first][tile_of_bucket]).astype(np.uint64)
        tile = np.repeat(tile_of_bucket, self.sizes)
        local = (np.repeat(rel, self.sizes) << np.uint64(22)) | (self.keys & np.uint64((1 << 22) - 1))
        bins = local >> np.maximum(0, 22 + seg[tile] - 12).astype(np.uint64)
        _, cnt = np.unique(tile.astype(np.uint64) << np.uint64(32) | bins, return_counts=True)
        _, where = np.unique(tile.astype(np.uint64) << np.uint64(32) | bins, return_index=True)
        return sorted(set(int(x) for x in tile[where[cnt > E.LS_KMAX]]))

    def tile_of_lead(self, lead):
        """(first slot, count) of the tile that holds the suffixes starting with this byte -- which must be all of it."""
        slots = np.flatnonzero(self.t[self.order] == lead)
        i = int(np.searchsorted(self.e0, slots[0], side='right')) - 1
        e0, c = int(self.e0[i]), int(self.counts[i])
        assert slots[0] == e0 and slots.size == c and slots[-1] == e0 + c - 1 and self.buckets[i] == 1, (lead, e0, c, slots.size)
        return e0, c

    def ties_in(self, e0, c):
        """Local positions of the tile whose key equals their predecessor's."""
        assert not self.tie[e0] and (e0 + c == self.n or not self.tie[e0 + c])        # groups never cross tiles
        return set(int(p) for p in np.flatnonzero(self.tie[e0:e0 + c]))

    def bins_in(self, e0, c):
        """(bin numbers, sizes, first local position) of a one-bucket tile: the top 12 of the 22 bits below the bucket."""
        b = (self.keys[e0:e0 + c] >> np.uint64(10)) & np.uint64(0xfff)
        v, first, cnt = np.unique(b, return_index=True, return_counts=True)
        return v, cnt, first


def _records(ties, c):
    """Local positions that owe a record: tied with the predecessor or the successor."""
    return {p for p in range(c) if p in ties or p + 1 in ties}


# ---- the cases -------------------------------------------------------------------------------------------------------

COUNT_TILES = (1, 511, 512, 513, 1024, 1025)


def counts_case():
    """Tiles of 1, 511, 512, 513, 1024 and 1025 elements, in this order in the suffix array, with ties
      512-tile   in its last two slots, the last key's low 22 bits equal to those of the first key of the next tile
      513-tile   in slots 0 | 1
      1024-tile  in its last two slots
      1025-tile  at 511 | 512 (two rows, two waves), at 5 | 6 and 517 | 518 (thread 5 and 6: ties in two rows), and no
                 other: most of its waves have no tie at all
    and none in the 1- and the 511-tile."""
    rng = np.random.default_rng(8101)
    x = 200000                                                       # the continuation the 512- and the 513-tile share
    spec = {1: conts(rng, 1), 511: conts(rng, 511), 512: conts(rng, 512, pairs=[510], hi=x, last=x),
            513: conts(rng, 513, pairs=[0], first=x), 1024: conts(rng, 1024, pairs=[1022]),
            1025: conts(rng, 1025, pairs=[5, 511, 517])}
    tiles = [(LEADS[i], spec[k]) for i, k in enumerate(COUNT_TILES)]
    t = assemble((1 << 17) + 77, 8102, tiles)
    v = View(t)
    got = {}
    for lead, vs in tiles:
        e0, c = v.tile_of_lead(lead)
        assert c == len(vs)
        got[c] = (e0, v.ties_in(e0, c))
    assert {c: ties for c, (_, ties) in got.items()} == {1: set(), 511: set(), 512: {511}, 513: {1}, 1024: {1023},
                                                         1025: {6, 512, 518}}
    for k in COUNT_TILES:
        assert int(np.count_nonzero(v.counts == k)) >= 1
    # the 512-tile ends where the 513-tile starts, and the two keys there differ in the lead alone
    e512, e513 = got[512][0], got[513][0]
    low = np.uint64((1 << 22) - 1)
    assert e512 + 512 == e513 and (v.keys[e513 - 1] & low) == (v.keys[e513] & low) and v.keys[e513 - 1] != v.keys[e513]
    # the 1025-tile: a wave without a record, a thread with records in two rows
    rec = _records(got[1025][1], 1025)
    waves = {(p % ROW) // WAVE for p in rec}
    assert len(waves) < ROW // WAVE
    rows_of = {}
    for p in rec:
        rows_of.setdefault(p % ROW, set()).add(p // ROW)
    assert any(len(r) >= 2 for r in rows_of.values())
    for p in (6, 512, 518):                                          # each a pair, not more
        assert v.m.size[v.order[got[1025][0] + p]] == 2
    assert v.slow_tiles() == []
    return t


def cap_case():
    """A tile of MSD_TILE_CAP = 8176 elements (two buckets of 4088 that start in one window: 15 full rows and one of 496)
    with a tie in its last two slots and one at 511 | 512, and a lone bucket of MSD_MAX_BUCKET = 4088."""
    rng = np.random.default_rng(8201)
    s2b = E.FILL70[22]                                               # code(S2) + 2: the next joint bucket under the same lead
    lone = conts(rng, E.MSD_MAX_BUCKET, pairs=[4086])
    lo, hi = conts(rng, 4088, pairs=[511]), conts(rng, 4088, pairs=[4086])
    n = E.MSD_WIN * 30 + E.MSD_TILE_CAP + 5                          # the pair's first slot: 5 slots into a window
    r = np.random.default_rng(8202)
    t = np.empty(n, np.uint8)
    t[:n - 1] = E._fill(r, E.FILL70, n - 1)
    t[n - 1] = E.NL
    # the byte BEFORE a copy goes round the alphabet: the suffixes that start there share [byte | lead | S1] and the bin
    # below it, 4088 / 70 < LS_KMAX of them per byte -- left to chance some byte would come up more than 64 times and
    # the tile of that bucket would be declined
    copies = []
    for lead, s2, vs in ((LEADS[0], S2, lone), (LEADS[1], S2, lo), (LEADS[1], s2b, hi)):
        copies += [bytes([E.FILL70[i % A], lead, S1, s2]) + _cont_bytes(c) for i, c in enumerate(vs)]
    pitch = 12                                                       # (12 264 copies in 192 501 bytes)
    assert 8 + pitch * len(copies) < n - 8
    for i, j in enumerate(r.permutation(len(copies))):
        t[8 + pitch * i:8 + pitch * i + 7] = np.frombuffer(copies[j], np.uint8)
    v = View(t)
    e0, c = v.tile_of_lead(LEADS[0])
    assert c == E.MSD_MAX_BUCKET and v.ties_in(e0, c) == {4087}
    i = len(v.e0) - 1                                                # the last tile: both buckets of the largest lead
    assert int(v.counts[i]) == E.MSD_TILE_CAP and int(v.buckets[i]) == 2 and int(v.e0[i]) == n - E.MSD_TILE_CAP
    assert int(v.e0[i]) % E.MSD_WIN == 5
    assert (v.t[v.order[n - E.MSD_TILE_CAP:]] == LEADS[1]).all()
    assert v.ties_in(int(v.e0[i]), E.MSD_TILE_CAP) == {512, 8175}
    assert int(v.counts.max()) == E.MSD_TILE_CAP
    assert v.slow_tiles() == []
    return t


BIN_MS = (8, 9, 64)


def _bin_tile_check(v, lead, k, m):
    e0, c = v.tile_of_lead(lead)
    assert c == k and not v.ties_in(e0, c)
    _, cnt, first = v.bins_in(e0, c)
    assert int(cnt[-1]) == m and int(first[-1]) == k - m and k - m >= (k - 1) // ROW * ROW      # the last bin: m members, all in the last row
    assert int(cnt[:-1].max()) <= LS_WINDOW                                                      # no other long bin
    return e0, c


def bins_case():
    """Three tiles of 600 elements (one full row and a row of 88) whose last bin has exactly 8, 9 and 64 members, all in
    the tail row: the ranking window holds the bin exactly, is one short of it, and LS_KMAX members finish in its loop."""
    rng = np.random.default_rng(8301)
    tiles = [(LEADS[i], bin_conts(rng, 600, m)) for i, m in enumerate(BIN_MS)]
    t = assemble((1 << 17) + 13, 8302, tiles)
    v = View(t)
    for (lead, vs), m in zip(tiles, BIN_MS):
        _bin_tile_check(v, lead, 600, m)
    assert v.slow_tiles() == []
    return t


def decline_case():
    """The same with a bin of LS_KMAX + 1 = 65 members: the fast kernel hands this one tile to the general kernel."""
    rng = np.random.default_rng(8401)
    tiles = [(LEADS[0], bin_conts(rng, 600, E.LS_KMAX + 1))]
    t = assemble((1 << 17) + 29, 8402, tiles)
    v = View(t)
    e0, _ = _bin_tile_check(v, LEADS[0], 600, E.LS_KMAX + 1)
    # that tile and no other (the suffixes one byte into the copies share a bucket's tile too, spread over two bins there)
    assert v.slow_tiles() == [int(np.searchsorted(v.e0, e0))]
    return t


CASES = {'counts': counts_case, 'cap': cap_case, 'bins': bins_case, 'decline': decline_case}
SLOW_TILES = {'counts': 0, 'cap': 0, 'bins': 0, 'decline': 1}
