"""Texts that put the run-length path and the closed form for periodic texts (pysubstringsearch_amd/csrc/rle_build.hip)
exactly on their limits (tests/test_rle_edges_gpu.py), and the numpy model those tests compare the build's statistics
with.  Everything here runs on the CPU; tests/test_rle_texts.py runs every generator for every parameter the GPU tests
use and holds model_sa() to the oracle on each of them.

model(t)          the run table, the 512 classes (byte, type), the ids, and the sizes that decide which expansion runs.
model_sa(t, r)    the suffix array the path's own algorithm yields from the ranks of the run heads.
period_model(t)   the word the head of the text repeats, how far the repetition goes, whether the closed form is taken.
period_blocks()   the rotation blocks and late slots of the closed form, read off a suffix array.

Every generator checks, before it returns, that the text holds what the case is about."""
from types import SimpleNamespace

import numpy as np

# ---- the constants of rle_build.hip the cases are built around ------------------------------------------------------
RL_TILE = 4096          # rle_build.hip: RL_TILE = RL_BLOCK * 16 = 256 * 16 bytes of text per workgroup (rle_count / rle_starts)
STRIP = 16              # run_start_mask16: one thread, one aligned strip of 16 bytes, four 32-bit words
CB = 64                 # rle_build.hip: CB, runs per block of the matrix walk (one wave)
CSEG = 64               # rle_build.hip: CSEG, blocks per segment of the column scan
CHUNK = 64              # col_count_kernel / col_scatter_kernel: ids per chunk (id0 = c * 64)
EX_IPT = 8              # rle_build.hip: EX_IPT, slots per thread of rle_expand_kernel
RS_TILE = 4096          # radix_sort.hip: RS_TILE; rle_suffix_array writes it as a literal (small = n <= 4096u)
COLUMNS_MIN_N = 4096    # rle_suffix_array: clause (a) of `columns`
NCLASS = 512            # rle_meta_kernel: s_max[512], class q = byte * 2 + type
# rle_build.h / sa_build.hip (Build::screen_text): the screen of the closed form
PERIOD_MAX = 1024       # kPeriodMax
PERIOD_TAIL_MAX = 1024  # kPeriodTailMax
PERIOD_PROBE = 8192     # kPeriodProbe; the screen starts at n >= 4 * kPeriodProbe
PERIOD_MIN_N = 4 * PERIOD_PROBE
EXTENT_IPT = 16         # period_extent_kernel: bytes per thread and grid stride (grid = CUs * 8 workgroups of 256)
FILL_IPT = 8            # period_fill_kernel: outputs per thread

# Two clauses that no text can be on the far side of, so none is planted:
#  (e) of `columns`, NB * nchunks < 2^31, follows from (d), NB * idpad * 4 <= n * 8: n < 2^32 gives NB * idpad < 2^33 and
#      nchunks = idpad / 64, so NB * nchunks < 2^27.
assert (2 * (2 ** 32 - 1)) // CHUNK < 2 ** 31
#  the `margin` clause of period_suffix_array, 4 * (2p + 2t + 1) <= m, follows from the screen's n >= 32768 for every word
#      p <= 1024 and tail t = n - m <= 1024: the left side is at most 4 * 4097 = 16388, the right at least 32768 - 1024.
assert 4 * (2 * PERIOD_MAX + 2 * PERIOD_TAIL_MAX + 1) <= PERIOD_MIN_N - PERIOD_TAIL_MAX


def _round_up(x, m):
    return (x + m - 1) // m * m


def from_runs(values, lengths):
    values, lengths = np.asarray(values), np.asarray(lengths)
    assert values.size == lengths.size and (lengths > 0).all() and (values[1:] != values[:-1]).all()
    return np.repeat(values.astype(np.uint8), lengths)


# ---- models ----------------------------------------------------------------------------------------------------------

def model(t, sort_knob=False):
    """What rle_suffix_array derives from the text before it expands (rle_build.hip, steps 1 and 2 and the head of step 3)."""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    n = int(t.size)
    assert n >= 2
    m = SimpleNamespace(n=n)
    # 1. run table (run_start_mask16: position 0 starts a run, and every byte that differs from the one before)
    m.start = np.flatnonzero(np.concatenate([[True], t[1:] != t[:-1]])).astype(np.int64)
    m.S = int(m.start.size)
    m.end = np.concatenate([m.start[1:], [n]]).astype(np.int64)
    m.byte = t[m.start].astype(np.int64)
    m.L = m.end - m.start
    # 2. rle_meta_kernel: type = (next byte > c); the end of the text is below every byte, so the last run is type 0
    nxt = np.where(m.end < n, t[np.minimum(m.end, n - 1)].astype(np.int64), -1)
    m.type = (nxt > m.byte).astype(np.int64)
    m.meta = (m.byte << 33) | (m.type << 32) | np.where(m.type == 1, (~m.L) & 0xffffffff, m.L)      # the 41-bit sort key
    m.cls = m.byte * 2 + m.type
    m.cls_max = np.zeros(NCLASS, np.int64)
    np.maximum.at(m.cls_max, m.cls, m.L)
    # rle_class_kernel: cls_base = exclusive sums, cls_base[512] = number of ids
    m.cls_base = np.concatenate([[0], np.cumsum(m.cls_max)]).astype(np.int64)
    m.num_ids = int(m.cls_base[NCLASS])
    # rle_runinfo_kernel / col_prep_kernel: type 0: id = base + r - 1, type 1: id = top - r with top = base + max; a run of L
    # bytes covers the ids [lo, hi)
    m.base = m.cls_base[m.cls]
    m.top = m.base + m.cls_max[m.cls]
    m.lo = np.where(m.type == 1, m.top - m.L, m.base)
    m.hi = np.where(m.type == 1, m.top, m.base + m.L)
    # rle_suffix_array: int id_bits = 1; while ((1ull << id_bits) < num_ids) ++id_bits;
    m.id_bits = 1
    while (1 << m.id_bits) < m.num_ids:
        m.id_bits += 1
    m.NB = (m.S + CB - 1) // CB
    m.idpad = _round_up(m.num_ids, CHUNK)
    m.nchunks = m.idpad // CHUNK
    m.nseg = (m.NB + CSEG - 1) // CSEG
    m.clauses = {'a': n >= COLUMNS_MIN_N, 'b': m.S * 4 <= n, 'c': m.idpad * 4 <= n, 'd': m.NB * m.idpad * 4 <= n * 8,
                 'e': m.NB * m.nchunks < 2 ** 31}
    m.columns = (not sort_knob) and all(m.clauses.values())
    m.small = n <= RS_TILE
    m.passes = (m.id_bits + 7) // 8
    return m


def head_ranks(t, sa):
    """Rank of every run head among the run heads, from a suffix array of the text."""
    m = model(t)
    isa = np.empty(m.n, np.int64)
    isa[np.asarray(sa, dtype=np.int64)] = np.arange(m.n)
    return np.argsort(np.argsort(isa[m.start]))


def naive_head_ranks(t):
    """The same by comparing the suffixes byte by byte (small texts: the generators' own checks)."""
    m = model(t)
    assert m.S * m.n <= 1 << 25
    raw = np.ascontiguousarray(t, dtype=np.uint8).tobytes()
    order = sorted(range(m.S), key=lambda k: raw[m.start[k]:])
    r = np.empty(m.S, np.int64)
    r[order] = np.arange(m.S)
    return r


def generation_order(m, ranks):
    """(SAr, j0, ord): rle_ord -- the last run first, then the predecessor of every SAr[j], j != j0 (run 0 has none)."""
    sar = np.argsort(np.asarray(ranks), kind='stable').astype(np.int64)
    j0 = int(np.flatnonzero(sar == 0)[0])
    order = np.concatenate([[m.S - 1], np.delete(sar, j0) - 1]).astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(m.S))
    return sar, j0, order


def model_sa(t, ranks):
    """The suffix array by the path's own algorithm (rle_build.hip, step 3): the suffixes in generation order, run after
    run and inside a run by position; the id of each; a stable sort by id alone."""
    m = model(t)
    _, _, order = generation_order(m, ranks)
    lens = m.L[order]
    off = np.concatenate([[0], np.cumsum(lens)])[:-1]
    run = np.repeat(order, lens)
    pos = np.repeat(m.start[order], lens) + (np.arange(m.n) - np.repeat(off, lens))
    r = m.end[run] - pos
    ids = np.where(m.type[run] == 1, m.top[run] - r, m.base[run] + r - 1)
    assert ids.min() >= 0 and ids.max() < m.num_ids
    return pos[np.argsort(ids, kind='stable')].astype(np.int32)


def period_of_head(head):
    """period_of_head (rle_build.hip): 0 for one byte repeated, else the smallest p in [2, 1024] with 4 p <= len and
    head[i] == head[i + p] for every i + p < len, else 0."""
    head = np.asarray(head, dtype=np.uint8)
    ln = int(head.size)
    if ln > 1 and (head == head[0]).all():
        return 0
    p = 2
    while p <= PERIOD_MAX and 4 * p <= ln:
        if np.array_equal(head[:ln - p], head[p:]):
            return p
        p += 1
    return 0


def period_model(t):
    """Build::screen_text / try_periodic (sa_build.hip), period_extent and the head of period_suffix_array.
    `period` and `extent` are what the statistics report: zero when the screen does not look or finds no word."""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    n = int(t.size)
    pm = SimpleNamespace(n=n, screened=n >= PERIOD_MIN_N)
    pm.p = period_of_head(t[:min(n, PERIOD_PROBE)])
    pm.m, pm.first = n, None
    if pm.p:
        diff = np.flatnonzero(t[:n - pm.p] != t[pm.p:])
        if diff.size:
            pm.first = int(diff[0])                     # what period_extent_kernel leaves in *first
            pm.m = pm.first + pm.p
    pm.tail = n - pm.m
    pm.margin = 2 * pm.p + 2 * pm.tail + 1
    pm.taken = bool(pm.screened and 2 <= pm.p <= PERIOD_MAX and pm.tail <= PERIOD_TAIL_MAX and 4 * pm.margin <= pm.m)
    pm.desc = bool(pm.p and (pm.m == n or t[pm.m] < t[pm.m % pm.p]))
    pm.period = pm.p if pm.screened else 0
    pm.extent = pm.m if pm.screened and pm.p else 0
    pm.long_end = pm.m - pm.margin if pm.taken else None
    return pm


def period_blocks(t, sa):
    """The block table period_suffix_array builds on the host, read off a suffix array instead of its sort: [(out, count,
    cls)] for the rotation blocks -- the long suffixes (position < long_end) of one class cls = position mod p, contiguous and
    ascending or descending by p -- and the slots of the late suffixes.  Asserts that the suffix array has this shape."""
    pm = period_model(t)
    assert pm.taken
    sa = np.asarray(sa, dtype=np.int64)
    late = sa >= pm.long_end
    cut = np.flatnonzero(np.concatenate([[True], late[1:] | late[:-1] | (sa[1:] % pm.p != sa[:-1] % pm.p)]))
    blocks = []
    for a, b in zip(cut, np.concatenate([cut[1:], [pm.n]])):
        if late[a]:
            assert b == a + 1
            continue
        seg = sa[a:b]
        cls = int(seg.min())
        assert cls < pm.p and seg.size == (pm.long_end - cls + pm.p - 1) // pm.p, (cls, seg.size)
        want = cls + pm.p * np.arange(seg.size)
        assert np.array_equal(seg, want[::-1] if pm.desc else want)
        blocks.append((int(a), int(seg.size), cls))
    assert sorted(b[2] for b in blocks) == list(range(min(pm.p, pm.long_end)))
    return blocks, np.flatnonzero(late)


# ---- run-length cases ------------------------------------------------------------------------------------------------

STRIP_DS = (-1, 0, 1)
STRIP_REMS = (0, 1, 15)
STRIP_XORS = (0x80, 0x01, 0xff)


def strip_case(d, rem=0):
    """run_start_mask16 on its strips.  Runs begin at every residue mod 16 -- so at every word boundary inside a strip,
    where the `prev` carry hands the last byte of one 32-bit word to the next, and at residue 0, where `prev` is a load --
    and at each residue the two neighbours differ only in bit 7, only in bit 0, and in all bits (the SWAR test for a
    non-zero byte).  A run begins exactly at RL_TILE * k + d for k = 1, 2 (d = -1: the last byte of a tile, 0: its first,
    1: its second) and nowhere else within one byte of it.  n % 16 = rem: 0 keeps every strip on the vector branch, 1 and 15
    send the last strip through the scalar branch, with a run that begins inside it.  (At a device pointer that is not
    16-byte aligned every strip takes the scalar branch, and sa_symbols_kernel, which counts the same runs a second way,
    its scalar loop: the build fails with "internal error" when the two counts differ.)  Bytes 0 and 255 occur."""
    assert d in STRIP_DS and rem in STRIP_REMS
    n = 2 * RL_TILE + 65 * STRIP + rem
    lens = ([17] * 48 + [1, 2, 1, 3, 1, 1, 4, 2, 5]) * (n // 800 + 1)
    is_start = np.zeros(n, bool)
    s = np.concatenate([[0], np.cumsum(lens)])
    is_start[s[s < n]] = True
    targets = [RL_TILE * k + d for k in (1, 2)]
    for x in targets:
        is_start[x - 2:x + 3] = False
        is_start[x] = True
    is_start[n - 3:] = [False, False, True]                     # a run of one byte ends the text: type 0, inside the last strip
    starts = np.flatnonzero(is_start)
    values = np.bitwise_xor.accumulate(np.array([0] + [STRIP_XORS[i % 3] for i in range(starts.size - 1)], np.uint8))
    t = from_runs(values, np.diff(np.concatenate([starts, [n]])))
    # the checks
    m = model(t)
    assert t.size == n and n % STRIP == rem and np.array_equal(m.start, starts)
    for x in targets:
        assert is_start[x] and not is_start[x - 2:x].any() and not is_start[x + 1:x + 3].any()
    vec = starts[(starts > 0) & (starts // STRIP * STRIP + STRIP <= n)]          # starts inside strips of the vector branch
    seen = {(int(t[x] ^ t[x - 1]), int(x % STRIP)) for x in vec}
    assert seen >= {(x, r) for x in STRIP_XORS for r in range(STRIP)}
    assert (rem == 0) == (n % STRIP == 0) and is_start[n - 1] and 0 in t and 255 in t
    return t


IDBITS_NS = (2, 256, 257, 65536, 65537)


IDBITS_BIG_NS = (2, 256, 257)


def idbits_case(num_ids, big=False):
    """Exactly num_ids ids: id_bits = 1, 8, 9, 16, 17 on the two sides of `while ((1 << id_bits) < num_ids)`.  Four long runs
    in the classes (0, type 1), (255, type 0), (97, type 0) and (97, type 1) -- bytes 0 and 255, cls_base behind an empty
    stretch of classes, both id formulas -- plus runs of one byte in (96, 1) and (98, 0) and short filler that raises no
    class's longest run.  The last run is type 0.  n is num_ids + 12 (2 for num_ids = 2): for 2, 256 and 257 ids that is at
    most 4096 bytes, where the sort expansion is the single-workgroup sort of the whole key (`small`, final_buf = 0) and the
    number of passes plays no part.  `big` (2, 256, 257 ids) adds filler up to more than 4096 bytes, so that the radix sort
    takes (id_bits + 7) / 8 = 1, 1 and 2 passes and final_buf = passes & 1 is 1, 1 and 0; 65536 and 65537 ids take 2 and 3
    passes as they are.  (sbase carries the type in bit 31 beside base or top; both stay below num_ids <= n < 2^31, so no
    text can reach that bit.)"""
    assert not big or num_ids in IDBITS_BIG_NS
    if num_ids == 2:
        t = np.resize(np.array([0, 255], np.uint8), 4200 if big else 2)
    else:
        q = (num_ids - 2) // 4
        A, B, C = q, q + 1, q - 1
        D = num_ids - 2 - A - B - C
        vals = [0, 255, 97, 96, 97, 98, 97, 96, 97, 98, 0, 255, 97, 98]
        lens = [A, B, C, 1, D, 1, 2, 1, 3, 1, 2, 1, 1, 1]
        if big:
            vals, lens = vals + [97, 98] * 400, lens + [10, 1] * 400
        t = from_runs(vals, lens)
    m = model(t)
    assert m.num_ids == num_ids and m.type[-1] == 0
    assert (1 << m.id_bits) >= num_ids and (m.id_bits == 1 or (1 << (m.id_bits - 1)) < num_ids)
    assert (RS_TILE < t.size <= RS_TILE + 700 and not m.small) if big else t.size <= num_ids + 12
    assert m.small == (t.size <= RS_TILE) and (big or m.small == (num_ids <= 257))
    return t


def _alternating(rng, S, values, lo, hi):
    """S runs over `values` (neighbours differ), lengths uniform in [lo, hi]."""
    v = np.empty(S, np.int64)
    v[0] = rng.integers(0, len(values))
    step = rng.integers(1, len(values), S)
    for i in range(1, S):
        v[i] = (v[i - 1] + step[i]) % len(values)
    return np.asarray(values)[v], rng.integers(lo, hi + 1, S)


COLUMNS_CLAUSES = ('a', 'b', 'c', 'd')


def _columns_pair(clause):
    if clause == 'a':
        # n = 4096 | 4095: 256 runs of 16 bytes, the last one byte shorter on the failing side
        vals = np.resize(np.array([97, 98, 99], np.uint8), 256)
        lens = np.full(256, 16)
        short = lens.copy()
        short[-1] -= 1
        return from_runs(vals, lens), from_runs(vals, short)
    if clause == 'b':
        # S * 4 <= n: 2048 runs in 8192 | 8191 bytes
        rng = np.random.default_rng(71)
        vals, lens = _alternating(rng, 2048, [0, 97, 255], 1, 7)
        lens[:] = 4
        lens[0::2] += rng.integers(-3, 4, 1024)
        lens[1::2] = 8 - lens[0::2]
        short = lens.copy()
        short[1000] -= 1
        return from_runs(vals, lens), from_runs(vals, short)
    if clause == 'c':
        # idpad * 4 <= n: two long runs make 2048 | 2049 ids (idpad 2048 | 2112) in 8192 | 8193 bytes; 16-byte filler
        vals = np.concatenate([[97, 98], np.resize(np.array([97, 98], np.uint8), 384)])
        lens = np.concatenate([[1000, 1048], np.full(384, 16)])
        more = lens.copy()
        more[0] += 1
        return from_runs(vals, lens), from_runs(vals, more)
    # (d) NB * idpad * 4 <= n * 8: S = 4096 runs (NB = 64), idpad = 1984, so the two sides meet at n = 32 * 1984 = 63488
    rng = np.random.default_rng(73)
    vals, lens = _alternating(rng, 4094, [10, 97, 98, 200], 12, 18)
    vals = np.concatenate([[5], vals[:2000], [6], vals[2000:]])
    lens = np.concatenate([[1000], lens[:2000], [1], lens[2000:]])
    # (bytes 5 and 6 are below the filler's: two classes of type 1 that hold one long run each)
    lens[2001] = 1984 - (model(from_runs(vals, lens)).num_ids - 1)
    delta = 32 * 1984 - int(lens.sum())
    room = np.flatnonzero((lens < 18) & (lens > 12) if delta > 0 else (lens > 13) & (lens < 18))[:abs(delta)]
    assert room.size == abs(delta)
    lens[room] += 1 if delta > 0 else -1                                # (no class's longest run moves)
    short = lens.copy()
    short[100] -= 1
    return from_runs(vals, lens), from_runs(vals, short)


def columns_case(clause, side):
    """One text on each side of clause (a) n >= 4096, (b) S * 4 <= n, (c) idpad * 4 <= n, (d) NB * idpad * 4 <= n * 8 of
    `columns` (rle_suffix_array): the two differ by one byte of one run's length, the `holds` side meets the clause with
    equality, and every other clause holds in both -- so the matrix walk runs on one side and the stable sort on the other."""
    assert clause in COLUMNS_CLAUSES and side in ('holds', 'fails')
    holds, fails = _columns_pair(clause)
    mh, mf = model(holds), model(fails)
    assert abs(mh.n - mf.n) == 1 and mh.S == mf.S and np.count_nonzero(mh.L != mf.L) == 1
    assert mh.columns and all(mh.clauses.values())
    assert [k for k, v in mf.clauses.items() if not v] == [clause] and not mf.columns
    assert {'a': mh.n == COLUMNS_MIN_N, 'b': mh.S * 4 == mh.n, 'c': mh.idpad * 4 == mh.n,
            'd': mh.NB * mh.idpad * 4 == mh.n * 8}[clause]
    assert COLUMNS_MIN_N - 1 <= min(mh.n, mf.n) and max(mh.n, mf.n) <= 1 << 17
    assert mh.S * 8 <= mh.n or clause == 'b'                   # (runs average 8 bytes or more, but where S * 4 meets n)
    return holds if side == 'holds' else fails


BLOCK_SS = (1, 2, 63, 64, 65, 4096, 4097, 8193)


def block_case(S):
    """Exactly S runs.  63, 64, 65: one block of CB = 64 runs with an idle lane, a full one, and a second block with 63 idle
    lanes.  4096, 4097, 8193: NB = 64, 65, 129 blocks, so nseg = 1, 2, 3 segments of CSEG = 64 blocks in the two-level column
    scan, the last with one block.  `columns` holds for all of these.  It cannot hold for S = 1 and S = 2: two neighbouring
    runs are never of one class, so with up to three runs every byte has an id of its own, num_ids = n, and clause (c)
    fails; those two go through the sort expansion (more than 4096 bytes: not the single-workgroup sort) and the case
    asserts that instead."""
    assert S in BLOCK_SS
    if S <= 2:
        t = from_runs([98, 97][:S], [4096 + S, 98][:S])
        m = model(t)
        assert m.S == S and m.num_ids == m.n and not m.clauses['c'] and not m.columns and not m.small
        return t
    rng = np.random.default_rng(500 + S)
    vals, lens = _alternating(rng, S, [0, 97, 98, 255], *((50, 80) if S < 100 else (5, 12)))
    t = from_runs(vals, lens)
    m = model(t)
    assert m.S == S and m.columns and m.NB == (S + 63) // 64 and m.nseg == {63: 1, 64: 1, 65: 1, 4096: 1, 4097: 2, 8193: 3}[S]
    assert (m.NB * CB - S) == {63: 1, 64: 0, 65: 63, 4096: 0, 4097: 63, 8193: 63}[S]
    return t


CHUNK_DS = (-1, 0, 1)


def chunk_case(d):
    """The `full` shortcut of col_count_kernel / col_scatter_kernel, mylo <= id0 && myhi >= id0 + 64.  Every run length is a
    multiple of 64 plus d, over three bytes (five classes), 256 runs (four blocks).  d = 0: every class base and so every
    [lo, hi) is a multiple of 64 -- a run covers a chunk of 64 ids entirely or not at all, every chunk takes the shortcut,
    and the ones at a run's first and last chunk take it with equality.  d = +-1: no run's [lo, hi) has both ends on a
    multiple of 64, so the chunks at its ends go through the per-id loop."""
    assert d in CHUNK_DS
    rng = np.random.default_rng(640 + d)
    vals, mult = _alternating(rng, 256, [0, 97, 255], 1, 4)
    t = from_runs(vals, mult * CHUNK + d)
    m = model(t)
    assert m.columns and m.NB == 4 and np.unique(m.cls).size >= 3 and ((m.L - d) % CHUNK == 0).all()
    aligned = (m.lo % CHUNK == 0) & (m.hi % CHUNK == 0)
    assert aligned.all() if d == 0 else not aligned.any()
    if d == 0:
        assert (m.cls_base % CHUNK == 0).all() and m.num_ids == m.idpad
    return t


J0_WHERES = ('first', 'last', 'middle')


def j0_case(where):
    """rle_ord skips slot j0, the place of run 0 in SAr (it has no predecessor): j0 = 0 (the text begins with the smallest
    run head: the longest type-1 run of byte 0), j0 = S - 1 (with the largest: the longest type-0 run of byte 255), and in
    between.  4200 bytes and up, so that both expansions run."""
    assert where in J0_WHERES
    rng = np.random.default_rng(90)
    vals, lens = _alternating(rng, 520, [0, 97, 255], 4, 12)
    head = {'first': ([0, 97], [40, 3]), 'last': ([255, 97], [40, 3]), 'middle': ([97, 0], [5, 3])}[where]
    if vals[0] == head[0][1]:
        vals, lens = vals[1:], lens[1:]
    t = from_runs(np.concatenate([head[0], vals]), np.concatenate([head[1], lens]))
    m = model(t)
    _, j0, _ = generation_order(m, naive_head_ranks(t))
    assert m.columns
    assert {'first': j0 == 0, 'last': j0 == m.S - 1, 'middle': m.S // 4 < j0 < 3 * m.S // 4}[where], (j0, m.S)
    return t


TINY_RS = (0, 1, 7)


def tiny_runs_case(r, small=False):
    """rle_expand_kernel: 8 slots of the generated sequence per thread.  Stretches of runs of 1 and 2 bytes, so one thread
    crosses 4 to 8 runs (its `while (p >= o1)` walk), after a binary search of off[]; n % 8 = r: 1 and 7 send the last
    thread through the scalar stores.  n = 4104, 4097, 4103, or with `small` 4096, 4089, 4095: the single-workgroup sort
    with the slot in the key, on both sides of `small = n <= 4096` (a literal that has to equal RS_TILE of radix_sort.hip) to
    the byte.  Three runs of 70, 50 and 33 bytes keep the ids apart from the slots.  Used under PSS_RLE=1: the runs average
    2 bytes."""
    assert r in TINY_RS
    n = (RS_TILE - 8 + r if r else RS_TILE) if small else (RS_TILE + r if r else RS_TILE + 8)
    rng = np.random.default_rng(800 + r + (50 if small else 0))
    vals, lens = _alternating(rng, n, [97, 98, 99], 1, 2)
    lens[:600] = 1                                                  # "abcacb...": eight runs per thread
    lens[[700, 1500, 2000]] = (70, 50, 33)
    cut = int(np.searchsorted(np.cumsum(lens), n))
    vals, lens = vals[:cut + 1].copy(), lens[:cut + 1].copy()
    lens[-1] -= int(lens.sum()) - n
    t = from_runs(vals, lens)
    m = model(t)
    assert m.n == n and n % EX_IPT == r and m.small == small and (small or not m.columns)
    assert (n == RS_TILE) if small and r == 0 else (n == RS_TILE + 1) if r == 1 and not small else True
    _, _, order = generation_order(m, naive_head_ranks(t))
    off = np.concatenate([[0], np.cumsum(m.L[order])])
    p0 = np.arange(0, n - EX_IPT + 1, EX_IPT)
    crossed = np.searchsorted(off, p0 + EX_IPT - 1, side='right') - np.searchsorted(off, p0, side='right') + 1
    assert {4, 5, 6, 7, 8} <= set(crossed.tolist()), sorted(set(crossed.tolist()))
    return t


def tier_case(k):
    """The group-size tiers of the rank rounds (sa_rounds_impl.h: GS_CAP 512, MID_CAP 4096, two tiles of 4096) in the mode
    only this path uses: suffix_rounds_integer runs the Rounds on the REDUCED string, without codes (rank_only) and from
    h0 = 1.  k units  a^5 b^4 c^3 d^2 x^i y^j x^l z  in random order: the k runs a^5 carry one meta symbol, so do the b^4, c^3
    and d^2 behind them (and the z before them), and only the three digit runs (i, j, l: different for every unit) tell the units apart.  The group
    of k run heads at a^5 is therefore still whole after the first rank round (h = 1 looks at b^4: all tied) and after the
    second (h = 2 looks at c^3, tied until then), and no larger group exists."""
    assert k >= 2
    base = 2
    while base ** 3 < k:
        base += 1
    rng = np.random.default_rng(4000 + k)
    ident = rng.permutation(base ** 3)[:k]
    digits = np.stack([ident % base, ident // base % base, ident // base // base], axis=1) + 1
    vals = np.tile(np.array([97, 98, 99, 100, 120, 121, 120, 122], np.uint8), k)
    lens = np.tile(np.array([5, 4, 3, 2, 0, 0, 0, 1]), (k, 1))
    lens[:, 4:7] = digits
    t = from_runs(vals, lens.reshape(-1))
    m = model(t)
    assert m.S == 8 * k and m.n <= 1 << 20
    _, counts = np.unique(m.meta, return_counts=True)
    assert int(counts.max()) == k and int(np.count_nonzero(counts == k)) == 5      # a, b, c, d and z
    heads = np.flatnonzero(m.meta == m.meta[0])
    assert heads.size == k and (heads % 8 == 0).all()
    for j in (1, 2, 3):
        assert np.unique(m.meta[heads + j]).size == 1                     # the next three symbols: tied in every unit
    assert np.unique(m.meta[heads[:, None] + np.arange(4, 7)], axis=0).shape[0] == k      # the digits: all different
    return t


# ---- closed-form cases -----------------------------------------------------------------------------------------------

def _word(seed, p):
    """A word of p letters b .. y whose repetition has no shorter period."""
    rng = np.random.default_rng(seed)
    while True:
        w = rng.integers(98, 122, p).astype(np.uint8)
        if period_of_head(np.resize(w, PERIOD_PROBE)) == p:
            return w


EXTENT_WHERES = ('16k-1', '16k', 'last', 'none')
_EXTENT_P = {'16k-1': 2, '16k': 40, 'last': 7, 'none': 13}


def extent_case(where, above=False):
    """period_extent_kernel: 16 positions i per thread, T[i] against T[i + p], an early `break`, atomicMin.  The first
    mismatch i = m - p is the last position of a thread's 16 (i % 16 = 15), the first of the next thread's (i % 16 = 0), the
    last position compared at all (i = n - p - 1: the break byte is the last byte of the text), or absent (m = n).  The break
    byte is one below the word's letter W[m % p] (descending blocks) or, with `above`, one above (ascending).  Words of 2, 40,
    7 and 13 letters, about 40 000 bytes, a tail of at most 612 bytes: the closed form is taken."""
    assert where in EXTENT_WHERES
    p = _EXTENT_P[where]
    n = 40000 + p
    t = np.resize(_word(300 + p, p), n).copy()
    if where != 'none':
        i = {'16k-1': 39407, '16k': 39408, 'last': n - p - 1}[where]
        t[i + p] = int(t[i + p]) + (1 if above else -1)
    pm = period_model(t)
    assert pm.p == p and pm.taken and model(t).S * 8 > n
    if where == 'none':
        assert pm.m == n and pm.first is None and pm.desc
    else:
        assert pm.first == i and pm.m == i + p and pm.desc == (not above)
        assert {'16k-1': i % EXTENT_IPT == 15, '16k': i % EXTENT_IPT == 0, 'last': i == n - p - 1 and pm.m == n - 1}[where]
    return t


def extent_far_case(cus):
    """The grid stride of period_extent_kernel: cus * 8 workgroups of 256 threads take 16 bytes each, so one stride is
    cus * 8 * 256 * 16 bytes (8 MiB at 256 compute units) and only a longer text sends any thread round its loop a second
    time -- nothing smaller reaches that code.  n = one stride + 5000; the break byte sits 500 bytes before the end, where
    only second-stride threads look (the first stride finds nothing and must not stop anybody), and the closed form is taken."""
    stride = cus * 8 * 256 * EXTENT_IPT
    n = stride + 5000
    p = 23
    t = np.resize(_word(323, p), n).copy()
    t[n - 500] = int(t[n - 500]) - 1
    pm = period_model(t)
    assert pm.p == p and pm.m == n - 500 and pm.first == n - 500 - p >= stride and pm.taken and pm.desc
    return t


FILL_KINDS = ('single', 'stretch')


def fill_case(sa_of, kind='single'):
    """period_fill_kernel: 8 consecutive outputs per thread, one search of the block table and a walk that leaves a block,
    skips the slots period_late_kernel fills, and enters the next block.
      single   the word aababa, no tail: a late suffix shorter than the word sorts by its own few bytes, away from the other
               late suffixes of its rotation, and lands alone between two rotation blocks.  Some group of 8 outputs holds,
               strictly inside, the end of one block, that single late slot and the start of the next block.
      stretch  a word of 5 letters and a tail of 3 bytes, 5 blocks and 20 late suffixes: a group of 8 outputs holds the end of
               one block, several late slots and the start of the next block.
    The length of the text is searched for until the block table says so.  That table restates the host sort of
    period_suffix_array, which needs the true order: sa_of is the oracle's suffix array function."""
    assert kind in FILL_KINDS
    first = 33000 if kind == 'single' else 40000
    for n in range(first, first + 64):
        if kind == 'single':
            t = np.resize(np.frombuffer(b'aababa', dtype=np.uint8), n).copy()
        else:
            t = np.resize(_word(305, 5), n).copy()
            t[n - 3:] = (110, 100, 105)
        pm = period_model(t)
        assert pm.taken and (pm.p, pm.tail) == ((6, 0) if kind == 'single' else (5, 3)) and model(t).S * 8 > n
        blocks, late = period_blocks(t, sa_of(t))
        if fill_group(blocks, late, n, kind) is not None:
            assert len(blocks) == pm.p and late.size == pm.n - pm.long_end == pm.margin + pm.tail
            return t
    raise AssertionError('no length puts the block boundary inside a group of 8 outputs')


def fill_group(blocks, late, n, kind):
    """The first output of a group of FILL_IPT outputs that holds, strictly inside (neither its first nor its last output),
    the last slot of one block, late slots -- exactly one for `single`, two or more for `stretch` -- and the first slot of
    the next block; None when the block table has no such group."""
    is_late = np.zeros(n, bool)
    is_late[late] = True
    ends = {b[0] + b[1] for b in blocks}                                   # one past the last slot of a block
    for o in sorted(b[0] for b in blocks):                                 # the first slot of a block
        g = o // FILL_IPT * FILL_IPT
        e = max([x for x in ends if x <= o], default=None)
        if e is None or e == o or not is_late[e:o].all():
            continue
        if (o - e == 1) == (kind == 'single') and g < e - 1 and o < g + FILL_IPT - 1:
            return g
    return None
