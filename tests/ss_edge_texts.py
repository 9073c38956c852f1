"""The sample sort (pysubstringsearch_amd/csrc/ss_sort_impl.h, ss_suffix_sort in msd_sort.hip) restated on the CPU, and
texts that put it on its limits.  tests/test_ss_edges_gpu.py compares the statistics of forced builds with this model;
tests/test_ss_edge_texts.py runs every generator and checks the model's own invariants without a GPU.

Everything the sort does before the local merge is a function of the text alone:

geometry()          ss_geometry: index bits ib (2^ib >= n), symbols per key kc (the largest kc <= 32 with
                    R^kc <= 2^(128 - ib)), B1 x B2 joint buckets of about 512 elements, os sample members per bucket,
                    S = os B1 B2 samples; the sort refuses n < 2^16 and 4 S > n.  R = sigma + 1, or 257 when all 256
                    byte values occur (the codes are then raw bytes + 1; 0 stands past the end either way).
elements()          (sum c_j R^(kc-1-j)) << ib | index as two uint64 columns (hi, lo), dense codes 1 .. sigma.
sample_positions()  ss_sample_kernel: sample i is a fixed hash of i (two multiply-xorshift steps) modulo the length of
                    stratum [i n / S, (i + 1) n / S), counted from the stratum's start.
Model               the rank of every element among all elements (no two are equal: the index is part of the number),
                    the sorted sample, and the JOINT BUCKET of every suffix: the number of j in 1 .. B1 B2 - 1 with
                    sorted_sample[j os] <= element -- the sample itself falls to the right.  That is the two-level
                    digit d1 * B2 + d2 of the kernels: the first-level splitters are sorted_sample[i spb], the second
                    level of first-level bucket d1 uses sorted_sample[d1 spb + i st2], and spb = os B2, st2 = os, so
                    both levels together count the splitters j os with j <= d1 B2 + d2.  Every bucket holds its own
                    os sample members, so none is empty and the sort reports B1 B2 buckets.
heads_*()           the three tile plans over the (non-empty) buckets: greedy on lengths rounded up to eight with cap
                    SS_TILE = 4096 (the default, ss_local_seg_kernel), greedy on plain lengths with cap SS_TILE_CAP =
                    4088 (PSS_SS_SEG=0), the window rule of msd_tile_head with SS_WIN = 3456 / cap 4088
                    (PSS_SS_WINDOW_PLAN=1).  tile_heads() of tests/sa_edge_texts.py has the MSD sort's window and cap
                    built in, so the rule is written out here with the two as arguments.
settle_steps()      per suffix, the first-level splitters that share its high 64-bit word and lie above it: the steps
                    ss_settle walks back (eight, then it bisects).
cell_shifts()       per first-level bucket, the shift csh ss_digits2_kernel derives from the span of its B2 - 1 splitters.
tied_heads()        the tile heads whose first element has the key bits of the element before it (ss_boundary_kernel).

The generators follow planted() / headed() of tests/sa_edge_texts.py; each asserts through the model that its text
holds what the case is about.  Every text ends in a newline."""
import numpy as np

from tests import sa_edge_texts as E

SS_MAX_CHARS = 32
SS_TILE = 4096
SS_TILE_CAP = 4088
SS_MAX_BUCKET = 4088
SS_WIN = 3456
SS_PLAN_SEG = 65536
SS_CELL_BITS = 12
MSD_TAG_SPAN = 2048          # the window rule starts a tile at every 2048th non-empty bucket whatever the windows say
HOST_SORT_MAX = 8192         # samples up to here are sorted on the host, more by two chained device radix sorts

NL = E.NL
LEAD = E.LEAD
LOWER = E.LOWER
FILL39 = E.FILL39
PLANS = ('seg', 'tile', 'window')            # default, PSS_SS_SEG=0, PSS_SS_WINDOW_PLAN=1
PLAN_ENV = {'seg': {}, 'tile': {'PSS_SS_SEG': '0'}, 'window': {'PSS_SS_WINDOW_PLAN': '1'}}


def geometry(n, radix):
    """ss_geometry as a dict, or None where the sort refuses the text."""
    if n < (1 << 16) or n > (1 << 30) or radix < 2 or radix > 257:
        return None
    ib = 1
    while (1 << ib) < n:
        ib += 1
    kc = 0
    while kc < SS_MAX_CHARS and radix ** (kc + 1) <= 1 << (128 - ib):
        kc += 1
    if kc < 2:
        return None
    key_bits = (radix ** kc - 1).bit_length()
    lb = 4
    while (512 << lb) < n and lb < 20:
        lb += 1
    B1, B2 = 1 << ((lb + 1) // 2), 1 << (lb // 2)
    os_ = 8 if n > 768 * B1 * B2 else 4
    S = os_ * B1 * B2
    if 4 * S > n:
        return None
    return dict(n=n, radix=radix, ib=ib, kc=kc, key_bits=key_bits, B1=B1, B2=B2, os=os_, S=S, spb=os_ * B2, st2=os_,
                zl=max(0, min(64 - SS_CELL_BITS, 128 - key_bits - ib)), hi_bits=min(64, max(1, key_bits + ib - 64)))


def codes_of(t):
    """(codes, radix): dense codes 1 .. sigma in byte order, or raw bytes + 1 when all 256 values occur."""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    present = np.unique(t)
    if present.size == 256:
        return t.astype(np.uint64) + np.uint64(1), 257
    lut = np.zeros(256, np.uint64)
    lut[present] = np.arange(1, present.size + 1, dtype=np.uint64)
    return lut[t], int(present.size) + 1


def elements(t, g=None):
    """(hi, lo) of every suffix's element; the key is built in four 32-bit limbs (a limb times R plus a carry fits 64 bits)."""
    codes, radix = codes_of(t)
    n = codes.size
    g = g or geometry(n, radix)
    assert g is not None and g['radix'] == radix and g['n'] == n
    kc, ib = g['kc'], g['ib']
    c = np.concatenate([codes, np.zeros(kc, np.uint64)])
    limb = [np.zeros(n, np.uint64) for _ in range(4)]
    R, m32 = np.uint64(radix), np.uint64(0xffffffff)
    for j in range(kc):
        carry = c[j:j + n]
        for i in range(4):
            v = limb[i] * R + carry
            limb[i] = v & m32
            carry = v >> np.uint64(32)
        assert not carry.any()
    klo = (limb[1] << np.uint64(32)) | limb[0]
    khi = (limb[3] << np.uint64(32)) | limb[2]
    hi = (khi << np.uint64(ib)) | (klo >> np.uint64(64 - ib))
    lo = (klo << np.uint64(ib)) | np.arange(n, dtype=np.uint64)
    assert not (khi >> np.uint64(64 - ib)).any()
    return hi, lo


def sample_positions(n, S):
    i = np.arange(S, dtype=np.uint64)
    s0 = i * np.uint64(n) // np.uint64(S)
    s1 = (i + np.uint64(1)) * np.uint64(n) // np.uint64(S)
    with np.errstate(over='ignore'):
        x = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(29)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(32)
    return (s0 + x % (s1 - s0)).astype(np.int64)


def positions_for(n, radix=28):
    """Sample positions of a text of n bytes (they do not depend on the alphabet as long as the sort takes the text)."""
    g = geometry(n, radix)
    return sample_positions(n, g['S'])


class Model:
    def __init__(self, t):
        t = np.ascontiguousarray(t, dtype=np.uint8)
        self.t = t
        self.n = n = t.size
        _, radix = codes_of(t)
        self.g = g = geometry(n, radix)
        assert g is not None, (n, radix)
        self.hi, self.lo = elements(t, g)
        self.order = np.lexsort((self.lo, self.hi))               # element order: slot -> suffix
        self.rank = np.empty(n, np.int64)
        self.rank[self.order] = np.arange(n)
        self.pos = sample_positions(n, g['S'])
        self.sample = np.sort(self.rank[self.pos])                 # the sorted sample, as ranks
        nb = g['B1'] * g['B2']
        self.splitters = self.sample[g['os']::g['os']]             # sorted_sample[j os], j = 1 .. nb - 1
        assert self.splitters.size == nb - 1
        self.bucket = np.searchsorted(self.splitters, self.rank, side='right')
        self.sizes = np.bincount(self.bucket, minlength=nb).astype(np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        # key bits only (everything above the index) of the element in every slot: equal neighbours are tied
        ib = np.uint64(g['ib'])
        shi, slo = self.hi[self.order], self.lo[self.order] >> ib
        self.tied = np.zeros(n, bool)                               # slot s holds the key bits of slot s - 1
        self.tied[1:] = (shi[1:] == shi[:-1]) & (slo[1:] == slo[:-1])

    # ---- what the build reports ----
    def stats(self, plan):
        return dict(ss_buckets=int(np.count_nonzero(self.sizes)), ss_max_bucket=int(self.sizes.max()),
                    ss_samples=self.g['S'], ss_tiles=int(self.heads(plan).sum()))

    def accepted(self):
        return int(self.sizes.max()) <= SS_MAX_BUCKET

    # ---- tile plans: heads over the non-empty buckets ----
    def heads(self, plan):
        sizes = self.sizes[self.sizes > 0]
        if plan == 'seg':
            return heads_greedy((sizes + 7) // 8 * 8, SS_TILE)
        if plan == 'tile':
            return heads_greedy(sizes, SS_TILE_CAP)
        assert plan == 'window'
        return heads_window(sizes, SS_WIN, SS_TILE_CAP)

    def tile_starts(self, plan):
        """First slot of every tile, and n."""
        sizes = self.sizes[self.sizes > 0]
        cs = np.concatenate([[0], np.cumsum(sizes)])
        return np.append(cs[:-1][self.heads(plan)], self.n)

    # ---- branches of the digit passes ----
    def settle_steps(self):
        """Per suffix: first-level splitters with the element's high word that are larger as full numbers."""
        g = self.g
        spl1 = self.sample[g['spb']::g['spb']]                       # B1 - 1 ranks
        spl1_hi = self.hi[self.order[spl1]]
        by_word = np.searchsorted(spl1_hi, self.hi, side='right')   # what the high-word search leaves
        d1 = np.searchsorted(spl1, self.rank, side='right')
        assert np.array_equal(d1, self.bucket // g['B2'])
        steps = by_word - d1
        assert (steps >= 0).all()
        return steps

    def cell_shifts(self):
        """Per first-level bucket: csh of ss_digits2_kernel."""
        g = self.g
        out = []
        for seg in range(g['B1']):
            a = self._number(self.sample[seg * g['spb'] + g['st2']])
            b = self._number(self.sample[seg * g['spb'] + (g['B2'] - 1) * g['st2']])
            bits = (b - a).bit_length()
            out.append(max(bits - SS_CELL_BITS, 0))
        return out

    def _number(self, rank):
        s = self.order[rank]
        return (int(self.hi[s]) << 64) | int(self.lo[s])

    def tied_heads(self, plan):
        """Slots at which a tile starts with the key bits of the element before it."""
        ts = self.tile_starts(plan)[1:-1]
        return ts[self.tied[ts]]

    def groups_cut(self, plan):
        """Groups of equal key bits cut by a border: (slots of bucket borders inside a tile, slots of tile borders), each
        with the slot range [a, b) of the group it cuts."""
        ts = self.tile_starts(plan)[1:-1]
        bs = np.setdiff1d(self.starts[1:-1][self.sizes[1:] > 0], ts)
        return [self._cut(s) for s in bs if self.tied[s]], [self._cut(s) for s in ts if self.tied[s]]

    def _cut(self, s):
        a = s
        while self.tied[a]:
            a -= 1
        b = s + 1
        while b < self.n and self.tied[b]:
            b += 1
        return int(s), int(a), int(b)


def heads_greedy(lengths, cap):
    """A tile is the longest run of consecutive buckets that fits the cap (a bucket alone always does)."""
    cs = np.concatenate([[0], np.cumsum(lengths)])
    ne = len(lengths)
    head = np.zeros(ne, bool)
    k = 0
    while k < ne:
        head[k] = True
        k = max(k + 1, int(np.searchsorted(cs, cs[k] + cap, side='right')) - 1)
    return head


def heads_window(sizes, win, cap):
    """msd_tile_head without the LSD order's bucket numbers: the buckets that start inside one window of `win` slots share
    a tile; when they hold more than `cap` together the window's last bucket goes alone; every 2048th bucket starts one."""
    ne = len(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cs = start[:-1]
    w = cs // win
    head = (np.arange(ne) % MSD_TAG_SPAN) == 0
    head[1:] |= w[1:] != w[:-1]
    last = np.ones(ne, bool)
    last[:-1] = w[1:] != w[:-1]
    first_of_window = np.searchsorted(cs, w * win, side='left')
    head |= last & (start[1:] - cs[first_of_window] > cap)
    return head


def straddled_segments(lengths, cap):
    """Segment ends of the greedy plan (multiples of SS_PLAN_SEG in the running sum of `lengths`) that lie strictly inside
    a tile, and the number of segments."""
    cs = np.concatenate([[0], np.cumsum(lengths)])
    head = heads_greedy(lengths, cap)
    ts = np.append(cs[:-1][head], cs[-1])
    nseg = -(-int(cs[-1]) // SS_PLAN_SEG)
    ends = np.arange(1, nseg) * SS_PLAN_SEG
    at = np.searchsorted(ts, ends, side='left')
    return [int(e) for e, i in zip(ends, at) if ts[i] != e], nseg


# ---- the cases -------------------------------------------------------------------------------------------------------

BUCKET_KS = (4087, 4088, 4089, 4090)
TAIL_DS = E.TAIL_DS
SETTLE_MS = (1, 7, 8, 9, 13)


def _random_text(rng, n, alphabet):
    t = np.empty(n, np.uint8)
    t[:n - 1] = E._fill(rng, alphabet, n - 1)
    t[n - 1] = NL
    return t


def bucket_case(k):
    """a. One joint bucket of exactly k elements, no other above 4087: random text over 26 letters with a run of LEAD (larger
    than every other byte) in which every sample position is overwritten by a letter.  No sampled suffix starts with LEAD,
    so all of them fall behind the last splitter; the run's length is found with the model."""
    n = (1 << 16) + (0, 5, 16, 37)[k - 4087]
    rng = np.random.default_rng(5000 + k)
    base = _random_text(rng, n, LOWER)
    pos = positions_for(n)
    at = 3001
    length = k - 400
    for _ in range(40):
        t = base.copy()
        t[at:at + length] = LEAD
        inside = pos[(pos >= at) & (pos < at + length)]
        t[inside] = LOWER[7]
        m = Model(t)
        got = int(m.sizes[-1])
        if got == k:
            break
        length += k - got
    assert got == k, (k, got)
    assert not (t[pos] == LEAD).any() and t[-1] == NL
    assert (m.bucket[t == LEAD] == m.sizes.size - 1).all()
    assert int(m.sizes[:-1].max()) <= 4087 and int(m.sizes.max()) == k
    return t


# b. name -> (sizes of the ADJACENT last buckets, tile heads among all but the guard under the two greedy plans)
#    A guard bucket of 4088 comes first wherever the planted buckets themselves could join a bucket before them: it
#    shares a tile with nothing of more than eight slots, so a tile of both greedy plans starts at the bucket behind it.
PACKED = {
    'pad4096':    ((4088, 2048, 2048), {'seg': (1, 0), 'tile': (1, 1)}),              # padded 4096: fits; plain 4096: does not
    'pad4104':    ((4088, 1361, 1361, 1361), {'seg': (1, 0, 1), 'tile': (1, 0, 0)}),  # padded 3 x 1368 = 4104; plain 4083
    'plain4088':  ((4088, 2044, 2044), {'seg': (1, 0), 'tile': (1, 0)}),              # plain 4088, padded 4096: both fit
    'plain4089':  ((4088, 2044, 2045), {'seg': (1, 0), 'tile': (1, 1)}),              # plain 4089; padded still 4096
    'full_small': ((600, 4088, 5), {'seg': (1, 0), 'tile': (1, 1)}),                  # 4088 + 8 slots = 4096; 4093 elements
    'big_small':  ((600, 4081, 7), {'seg': (1, 0), 'tile': (1, 0)}),                  # padded 4088 + 8; plain 4088
}
_GROUP_BYTES = (b'abcdef', b'ghijkl', b'mnopqr', b'stuvwx')   # second byte of a group's heads


def packed_case(name):
    """b. Adjacent buckets of exactly the given sizes at the end of the suffix array: group g is the suffixes that start
    with LEAD and a letter of _GROUP_BYTES[g] (six letters each, so that the suffixes one byte on spread over the fill's
    own buckets).  Exactly os copies per group stand at sample positions, with the group's first letter and 'aaa' behind
    it; every other copy goes on with a letter above 'a' and stands clear of the sample positions.  The os sampled
    suffixes are then the smallest of their group, the sorted sample has a splitter on each group's first element, and
    the group is a bucket of its own."""
    sizes, want = PACKED[name]
    n = (1 << 17) + 3 + 2 * list(PACKED).index(name)
    rng = np.random.default_rng(6000 + list(PACKED).index(name))
    t = _random_text(rng, n, LOWER)
    g = geometry(n, 29)
    pos = sample_positions(n, g['S'])
    taken = np.zeros(n + 16, bool)
    for p in pos:
        taken[max(p - 8, 0):p + 1] = True                  # a copy that starts here would cover a sample position
    chosen = pos[5:5 + 11 * len(sizes) * g['os']:11]      # sampled copies: os per group
    for p in chosen:
        taken[p - 8:p + 8] = True
    at = 16
    for gi, c in enumerate(sizes):
        letters = _GROUP_BYTES[gi]
        for p in chosen[gi * g['os']:(gi + 1) * g['os']]:
            t[p:p + 5] = np.frombuffer(bytes([LEAD, letters[0]]) + b'aaa', dtype=np.uint8)
        left = c - g['os']
        while left:
            if not taken[at]:
                t[at:at + 3] = [LEAD, letters[int(rng.integers(len(letters)))], LOWER[1 + int(rng.integers(25))]]
                left -= 1
            at += 8
            assert at < n - 16
    m = Model(t)
    assert m.g['os'] == g['os'] and np.array_equal(m.pos, pos)
    assert tuple(m.sizes[-len(sizes):]) == sizes, (name, m.sizes[-len(sizes):])
    assert int((t[pos] == LEAD).sum()) == len(sizes) * g['os'] and m.accepted()
    for plan in ('seg', 'tile'):
        assert tuple(m.heads(plan)[-len(sizes) + 1:].astype(int)) == want[plan], (name, plan, m.heads(plan)[-len(sizes) - 1:])
    return t


def wordlike(rng, n, vocabulary=400):
    """Words of 2 .. 9 letters drawn with a skewed distribution, single blanks between them, n bytes, newline at the end."""
    words = [bytes(LOWER[int(c)] for c in rng.integers(0, 26, int(rng.integers(2, 10)))) for _ in range(vocabulary)]
    weight = 1.0 / np.arange(1, vocabulary + 1)
    pick = rng.choice(vocabulary, size=n // 3 + 8, p=weight / weight.sum())
    t = np.frombuffer(b' '.join(words[int(i)] for i in pick), dtype=np.uint8)[:n].copy()
    t[n - 1] = NL
    return t


def segments_case():
    """c. Word-like text of 300 007 bytes: 1024 buckets whose padded lengths fill more than four segments of SS_PLAN_SEG
    slots (five: three levels of jump tables), and at least one tile of the greedy plans lies across a segment's end."""
    t = wordlike(np.random.default_rng(7000), 300007)
    m = Model(t)
    assert m.accepted()
    cut, nseg = straddled_segments((m.sizes + 7) // 8 * 8, SS_TILE)
    assert nseg > 4 and (nseg - 1).bit_length() >= 3 and len(cut) >= 1, (nseg, cut)
    cut, nseg = straddled_segments(m.sizes, SS_TILE_CAP)
    assert nseg > 4 and len(cut) >= 1, (nseg, cut)
    return t


def settle_case(m_want):
    """d. 2^16 bytes over 26 letters with one run of 'q' (PSS_RLE=0 keeps the build on the sort): the suffixes inside the
    run have one key and differ in the index alone, a first-level splitter falls into every 4096 bytes of it, and the
    run's first suffix has all of them above it.  The run's length is found with the model: the most steps ss_settle walks
    for any suffix is exactly m_want."""
    n = 1 << 16
    rng = np.random.default_rng(8000 + m_want)
    base = _random_text(rng, n, LOWER)
    at = 777
    length = max(2048, (m_want - 1) * 4096 + 1024)
    for _ in range(24):
        t = base.copy()
        t[at:at + length] = ord('q')
        m = Model(t)
        got = int(m.settle_steps().max())
        if got >= m_want:
            break
        length += 512
    assert got == m_want and at + length < n - 64, (m_want, got, length)
    assert m.accepted() and t[-1] == NL
    if m_want >= 2:
        # a first-level bucket that lies inside the run: its B2 - 1 = 7 splitters are 512 bytes of run apart, index bits only
        assert 0 in m.cell_shifts()
    return t


def shift_case(name):
    """d, the shift cases of ss_cell_of.  'two': a two-letter text of 2^17 + 3 bytes -- keys of 32 two-bit symbols, 64 key
    bits above 18 index bits, so the B2 - 1 splitters of a first-level bucket span some 2^72 .. 2^80 numbers: buckets with
    0 < csh < 64, with csh > 64 and, reachable at this size, with csh == 64 exactly (a span of 76 bits).  'all': a text
    over all 256 byte values (105 key bits: csh beyond 100 everywhere).  csh == 0 comes from the runs of settle_case()."""
    rng = np.random.default_rng(8100)
    if name == 'two':
        t = _random_text(rng, (1 << 17) + 3, b'ab')
        shifts = Model(t).cell_shifts()
        assert 64 in shifts and any(0 < s < 64 for s in shifts) and any(s > 64 for s in shifts), sorted(set(shifts))
    else:
        t = _random_text(rng, (1 << 18) + 5, bytes(c for c in range(256) if c != NL))
        shifts = Model(t).cell_shifts()
        assert np.unique(t).size == 256 and min(shifts) > 64, sorted(set(shifts))
    return t


def ties_case():
    """e. planted(): a word of 300 symbols at 100 places, every position up to kc symbols before its end a group of 100
    elements with equal key bits in index order.  Under each plan at least one group is cut by a bucket border inside a
    tile and at least one by a tile border (Model.groups_cut)."""
    rng = np.random.default_rng(9000)
    word = E.make_word(rng, FILL39, 300)
    t = E.planted(rng, (1 << 17) + 11, FILL39, word, 100)
    m = Model(t)
    assert m.accepted()
    for plan in PLANS:
        inner, outer = m.groups_cut(plan)
        assert sum(b - a == 100 for _, a, b in inner) >= 1 and sum(b - a == 100 for _, a, b in outer) >= 1, (plan, len(inner), len(outer))
    return t


ALL_BUT_NL = bytes(c for c in range(256) if c != NL)


def tail_case(d, wide):
    """f. The last of 70 copies of a word ends d bytes before the final newline; the length is no multiple of 16.  Over 39
    symbols, or over all 256 byte values (raw bytes + 1 in the key, the packer tells the end of the text by the index).
    Over 39 symbols the length is also chosen so that the last stratum's sample lies in the last kc bytes: its key runs
    past the end of the text."""
    rng = np.random.default_rng(9500 + d + (100 if wide else 0))
    alphabet = ALL_BUT_NL if wide else FILL39
    word = E.make_word(rng, alphabet, 90)
    n = (1 << 16) + 1 + 2 * d + (1 << 15 if wide else 0)
    if not wide:
        g = geometry(n, 41)
        while n % 16 == 0 or positions_for(n)[-1] < n - g['kc']:
            n += 1
        assert geometry(n, 41)['kc'] == g['kc']
    assert n % 16
    t = E.planted(rng, n, alphabet, word, 70, tail=d)
    m = Model(t)
    assert m.accepted() and m.g['radix'] == (257 if wide else 41)
    if not wide:
        assert m.pos[-1] >= n - m.g['kc']
    return t


def unplanted_case(name):
    """Texts nothing is planted in, 2^16 .. 2^18 bytes: random over 2, 27 and 256 symbols, word-like, and the `words`
    corpus of the benchmark (tests/util.gen_corpus)."""
    rng = np.random.default_rng(9900)
    if name == 'random2':
        return _random_text(rng, (1 << 16) + 9, b'ab')
    if name == 'random27':
        return _random_text(rng, (1 << 18) - 3, LOWER)
    if name == 'random256':
        return _random_text(rng, (1 << 17) + 77, ALL_BUT_NL)
    if name == 'wordlike':
        return wordlike(rng, 200001)
    assert name == 'corpus1'
    from tests.util import gen_corpus
    t = np.array(gen_corpus(1, 1 << 18), dtype=np.uint8)
    t[-1] = NL
    return t


UNPLANTED = ('random2', 'random27', 'random256', 'wordlike', 'corpus1')


def device_sorted_case(name):
    """2^20 + 4097 bytes and a little more: S = 16 384 samples, more than the host sorts, so the sample goes through the two
    chained device radix sorts (64 bits of the low word, then hi_bits of the high word: 21 for the two-letter text, 62 for
    the text over all 256 byte values)."""
    rng = np.random.default_rng(9950)
    if name == 'two':
        t = _random_text(rng, (1 << 20) + 4097, b'ab')
    else:
        t = _random_text(rng, (1 << 20) + 4109, ALL_BUT_NL)
    g = geometry(t.size, codes_of(t)[1])
    assert g['S'] == 16384 > HOST_SORT_MAX and g['hi_bits'] == (21 if name == 'two' else 62)
    return t
