"""The LSD radix sort (pysubstringsearch_amd/csrc/radix_sort.hip) restated in numpy, and the texts that put its
flag-carrying passes on every route a tie flag can take (tests/test_lsd_edges_gpu.py).  Everything here runs on the
CPU; tests/test_lsd_texts.py holds the model to a brute force and every planted text to the routes it is meant to walk.

geometry(n, cap)       tiles, tiles per range and ranges of one pass.
pack_keys(...)         the sort keys the first pass packs from the recoded text (text_keys.h).
want_pairs(...)        radix_sort_pairs: the stable sort by the digits the pass mask keeps.
read_order(n)          the order in which the pass over the text ranks the suffixes of a tile (not by index).
want_suffix(...)       suffix_sort_flags / the plain passes over the text: one stable argsort, and "equals predecessor".
replay(...)            the passes one by one as the kernels take them: the order after every pass, the tie flag of every
                       element derived from the group numbers Z of the PREVIOUS pass's flags (never from the keys), and the
                       route by which each element found its predecessor.
census(...)            per pass, the elements on each route, tied and not tied.
planted(...)           skewed texts on which every route is walked both ways.

A pass moves element x behind y, the last element before it (in the order the pass reads) with the same digit.  The
kernel learns whether x and y agreed on the digits consumed so far by one of five routes:

in_tile      y sits in the same tile of 4096: neighbours in the tile's LDS exchange (exz[p - 1] == z).
carry        y sits in the previous tile of the same range: the digit's last group number, published by the tile before (s_tz).
carry_skip   y sits two or more tiles back in the same range: the tiles in between lack the digit and carry s_tz / s_tv forward.
fix          y sits in the previous range: fs_fix compares last_z of that range with first_z of this one.
fix_skip     y sits two or more ranges back: fs_fix looks back over ranges without the digit, adding their group heads (zeros[])."""
import numpy as np

# ---- the constants of radix_sort.hip the cases are built around -----------------------------------------------------
RS_TILE = 4096          # RS_BLOCK * RS_IPT = 256 * 16 elements per tile; up to it, pairs go to the one-workgroup sort
RS_MAX_RANGES = 1024    # the cap every build uses; the ranges of a pass are rounded up to a multiple of RANGE_ROUND
RANGE_ROUND = 8

ROUTES = ('in_tile', 'carry', 'carry_skip', 'fix', 'fix_skip')
U64 = np.uint64


def geometry(n, max_ranges=RS_MAX_RANGES):
    """(num_tiles, tiles_per_range, num_ranges) of a pass over n elements (rs_geometry)."""
    assert max_ranges % RANGE_ROUND == 0 and RANGE_ROUND <= max_ranges <= RS_MAX_RANGES
    num_tiles = (n + RS_TILE - 1) // RS_TILE
    tpr = (num_tiles + max_ranges - 1) // max_ranges
    used = (num_tiles + tpr - 1) // tpr if tpr else 0
    return num_tiles, tpr, (used + RANGE_ROUND - 1) // RANGE_ROUND * RANGE_ROUND


def _low(bits):
    return U64((1 << bits) - 1) if bits < 64 else U64(0xffffffffffffffff)


def passes_of(key_bits):
    return (key_bits + 7) // 8


def pack_keys(codes, n, b, k, plus_one, drop):
    """Key of every suffix i < n: k symbols of b bits, first symbol highest, zero past the end of the text, symbol =
    byte + 1 inside the text when plus_one; shifted right by drop.  Whatever `codes` holds past n is not looked at."""
    assert 1 <= k <= 16 and k * b <= 64 and 0 <= drop < b
    sym = np.zeros(n + k, dtype=U64)
    sym[:n] = np.asarray(codes[:n], dtype=U64) + U64(1 if plus_one else 0)
    assert int(sym.max(initial=0)) < (1 << b)
    key = np.zeros(n, dtype=U64)
    for j in range(k):
        key |= sym[j:j + n] << U64(b * (k - 1 - j))
    return key >> U64(drop)


def digit_mask(key_bits, pass_mask):
    m = 0
    for p in range(passes_of(key_bits)):
        if (pass_mask >> p) & 1:
            m |= 0xff << (8 * p)
    return U64(m)


def want_pairs(keys, vals, key_bits, pass_mask=0xffffffff):
    """The pairs in the order radix_sort_pairs leaves them: stable by the digits p < ceil(key_bits / 8) the mask keeps."""
    order = np.argsort(keys & digit_mask(key_bits, pass_mask), kind='stable')
    return keys[order], vals[order]


def read_order(n):
    """The order in which the pass over the TEXT ranks its elements.  A thread packs the keys of 16 consecutive suffixes
    (suffix = tile * 4096 + thread * 16 + r) and the wave ranks them round by round, r = 0 .. 15, all lanes at once: inside
    a tile equal digits leave by (wave, r, lane), not by index.  Every later pass reads what the pass before wrote, in
    order, and is stable -- so suffixes with equal keys end up in THIS order (nothing downstream of the sort looks at the
    order inside a group of equal keys; the model has to, it compares element by element)."""
    in_tile = np.arange(RS_TILE).reshape(RS_TILE // 1024, 64, 16).transpose(0, 2, 1).ravel()
    tiles = (n + RS_TILE - 1) // RS_TILE
    order = (np.arange(tiles)[:, None] * RS_TILE + in_tile[None, :]).ravel()
    return order[order < n]


def want_suffix(keys, key_bits, flags=True):
    """Suffix indices sorted by the whole digits that cover the low key_bits of the key, equal keys in read_order(); with
    flags, bit 31 of an entry says that its key (those digits of it) equals its predecessor's."""
    first = read_order(keys.size)
    m = (keys & _low(8 * passes_of(key_bits)))[first]
    by_key = np.argsort(m, kind='stable')
    order = first[by_key]
    m = keys & _low(8 * passes_of(key_bits))
    out = order.astype(np.uint32)
    if flags:
        s = m[order]
        out[1:] |= (s[1:] == s[:-1]).astype(np.uint32) << np.uint32(31)
    return out


def replay(keys, key_bits, max_ranges=RS_MAX_RANGES):
    """The flag-carrying passes one by one.  Returns a list with one entry per pass: (out, route, tied) where out is the
    pass's output (indices, bit 31 = flag), and route / tied say for every OUTPUT position how the element found its
    predecessor (index into ROUTES, -1: first of its digit) and whether the group numbers agreed."""
    n = keys.size
    _, tpr, _ = geometry(n, max_ranges)
    perm = read_order(n).astype(np.int64)          # (a permutation inside every tile: tiles and ranges are those of the index)
    flag = np.zeros(n, dtype=bool)
    out = []
    for p in range(passes_of(key_bits)):
        d = ((keys[perm] >> U64(8 * p)) & U64(0xff)).astype(np.uint8)       # (8-bit array: numpy radix-sorts it)
        order = np.argsort(d, kind='stable')
        # Z: heads up to and including the element, in the order the pass reads.  Nothing is consumed before pass 0.
        z = np.cumsum(~flag) if p else np.zeros(n, dtype=np.int64)
        ds = d[order]
        has_pred = np.concatenate([[False], ds[1:] == ds[:-1]])
        px, py = order, np.concatenate([[0], order[:-1]])
        tx, ty = px // RS_TILE, py // RS_TILE
        rx, ry = tx // tpr, ty // tpr
        route = np.where(tx == ty, 0, np.where(rx == ry, np.where(tx - ty == 1, 1, 2), np.where(rx - ry == 1, 3, 4)))
        route = np.where(has_pred, route, -1)
        tied = has_pred & (z[px] == z[py])
        perm, flag = perm[order], tied
        out.append((perm.astype(np.uint32) | (tied.astype(np.uint32) << np.uint32(31)), route, tied))
    return out


def census(keys, key_bits, max_ranges=RS_MAX_RANGES):
    """Per pass {route: (not tied, tied)}; plus the trailing empty ranges and the size of the last tile."""
    n = keys.size
    num_tiles, tpr, num_ranges = geometry(n, max_ranges)
    per_pass = []
    for _, route, tied in replay(keys, key_bits, max_ranges):
        c = np.bincount(route[route >= 0] * 2 + tied[route >= 0], minlength=2 * len(ROUTES))
        per_pass.append({name: (int(c[2 * i]), int(c[2 * i + 1])) for i, name in enumerate(ROUTES)})
    return per_pass, num_ranges - (num_tiles + tpr - 1) // tpr, n - (num_tiles - 1) * RS_TILE


def census_ok(per_pass):
    """The conditions a planted text must meet (tests/test_lsd_texts.py); returns what is missing."""
    missing = []
    for name in ROUTES:
        if sum(per_pass[0][name]) == 0:
            missing.append((0, name))
    for p in range(1, len(per_pass)):
        for name in ('in_tile', 'carry', 'fix'):
            for t in (0, 1):
                if per_pass[p][name][t] == 0:
                    missing.append((p, name, t))
    for name in ('carry_skip', 'fix_skip'):
        for t in (0, 1):
            if len(per_pass) > 1 and sum(c[name][t] for c in per_pass[1:]) == 0:
                missing.append(('any', name, t))
    return missing


# ---- texts ----------------------------------------------------------------------------------------------------------

# (code_bits, key_chars, drop, plus_one) of the flag passes' cases: every code width, keys of 9 .. 64 bits
CONFIGS = ((2, 16, 0, 0), (2, 16, 1, 0), (3, 16, 2, 0), (4, 16, 3, 0), (5, 12, 4, 0), (6, 10, 5, 0), (7, 9, 6, 0), (8, 8, 0, 0),
           (8, 8, 7, 0), (9, 7, 0, 1), (9, 7, 8, 1), (9, 2, 0, 1), (8, 2, 7, 0), (2, 5, 1, 0))
WIDEST = ((2, 16, 0, 0), (3, 16, 2, 0), (4, 16, 3, 0), (5, 12, 4, 0), (6, 10, 5, 0), (7, 9, 6, 0), (8, 8, 0, 0), (9, 7, 0, 1))
NO_FLAGS_CONFIGS = ((2, 16, 1, 0), (6, 10, 5, 0), (9, 7, 0, 1))
SWEEP = (9, 16, 17, 24, 33, 40, 41, 48, 49, 56, 57, 64)
PLANTED_NS = (65537, 69631, 98304, 98305)        # at cap 8: 3, 3, 3 and 4 tiles per range; a last tile of 1, 4095, 4096, 1
CAP = 8
PAD = 64


def key_width(cfg):
    b, k, drop, _ = cfg
    return k * b - drop


def sweep_of(cfg):
    """The key_bits a case runs at: its own width, and for the widest key of an alphabet every prefix of SWEEP below it."""
    w = key_width(cfg)
    return tuple(s for s in SWEEP if s < w) + (w,) if cfg in WIDEST else (w,)


def padded(codes, plus_one):
    """The text as the device wants it: PAD bytes behind it, zero -- or 0xFF where the kernels must not look (plus_one)."""
    return np.concatenate([np.asarray(codes, dtype=np.uint8), np.full(PAD, 0xFF if plus_one else 0, dtype=np.uint8)])


def alphabet(b, plus_one):
    """The byte values a text of this code width may hold: 1 .. 2^b - 1 (0 is the padding), any byte with plus_one."""
    return np.arange(0, 256, dtype=np.uint8) if plus_one else np.arange(1, 1 << b, dtype=np.uint8)


def _mixed(n, b, plus_one, seed):
    """Runs of one to three common symbols (groups of equal consumed digits that span whole tiles) with up to ten rarer
    symbols sprinkled over them, 2 .. 150 copies each: digits absent from whole tiles, and from whole ranges."""
    rng = np.random.default_rng([seed, b, plus_one])
    perm = rng.permutation(alphabet(b, plus_one))
    ncommon = int(rng.integers(1, min(3, perm.size - 1) + 1))
    mean_run = int(rng.choice([3, 40, 1500, 9000]))
    weights = rng.dirichlet(np.full(ncommon, 0.6)) if ncommon > 1 else np.ones(1)
    nruns = max(4, 2 * n // mean_run)
    lens = rng.geometric(1.0 / mean_run, nruns)
    t = np.repeat(perm[rng.choice(ncommon, nruns, p=weights)], lens)
    while t.size < n:
        t = np.concatenate([t, t])
    t = t[:n].copy()
    for s in perm[ncommon:ncommon + 10]:
        t[rng.choice(n, int(rng.choice([2, 3, 4, 6, 10, 16, 24, 40, 90, 150])), replace=False)] = s
    return t


def _runs(n, b, plus_one, seed):
    """Three to ten stretches, each repeating a word of one to three symbols, with up to six symbols per stretch changed in
    their top bit: the top digit of a short key then has two or three values, one of them rare inside a large group."""
    rng = np.random.default_rng([seed, b, plus_one, 2])
    a = alphabet(b, plus_one)
    ok = np.zeros(256, dtype=bool)
    ok[a] = True
    top = 0x80 if plus_one else 1 << (b - 1)
    m = int(rng.integers(3, 11))
    lens = np.maximum(1, (rng.dirichlet(np.full(m, 0.7)) * n).astype(np.int64))
    lens[-1] = max(1, n - int(lens[:-1].sum()))
    parts = []
    for ln in lens:
        w = a[rng.integers(0, a.size, int(rng.integers(1, 4)))]
        seg = np.tile(w, int(ln) // w.size + 1)[:int(ln)].copy()
        for at in rng.integers(0, int(ln), int(rng.integers(0, 7))):
            if ok[seg[at] ^ top]:
                seg[at] ^= top
        parts.append(seg)
    t = np.concatenate(parts)[:n]
    if t.size < n:
        t = np.concatenate([t, np.full(n - t.size, a[0], dtype=np.uint8)])
    return t.astype(np.uint8)


def _sprinkled(n, b, plus_one, seed):
    """Two to four common symbols drawn independently, their top-bit partners and three more symbols sprinkled 3 .. 50 times."""
    rng = np.random.default_rng([seed, b, plus_one, 1])
    a = alphabet(b, plus_one)
    perm = rng.permutation(a)
    ncommon = int(rng.integers(2, min(4, perm.size - 1) + 1))
    commons = perm[:ncommon]
    t = commons[rng.choice(ncommon, n, p=rng.dirichlet(np.full(ncommon, 1.5)))].astype(np.uint8)
    top = 1 << (b - 1)
    have, common = set(a.tolist()), set(commons.tolist())
    rare = [int(c) ^ top for c in commons if (int(c) ^ top) in have and (int(c) ^ top) not in common]
    rare += [int(s) for s in perm[ncommon:ncommon + 3] if int(s) not in rare]
    for s in rare:
        t[rng.choice(n, int(rng.choice([3, 5, 8, 12, 20, 30, 50])), replace=False)] = s
    return t


# Three texts placed by hand (by a search over stretch lengths, with the census as its only judge): a 9-bit key leaves the
# second pass ONE bit, and a range lacks a digit only where a stretch of equal low digits covers it whole.
# (word, length, positions whose symbol has its top bit changed) per stretch.
_SPECS = {
    0: (((3, 1, 3), 19394, (1485, 10517)), ((3,), 20464, (19785,)), ((1,), 25679, (11462,))),         # n = 65537
    1: (((3, 1, 3), 19394, (1485, 10517)), ((3,), 24048, (23369,)), ((1,), 26189, (11972,))),         # n = 69631
    2: (((1,), 54343, (821, 19589, 25851)), ((3, 2, 3), 119, (8, 44)),
        ((2, 3, 1), 43843, (13810, 16975, 17455, 22088, 33355, 39518))),                              # n = 98305
}


def _spec(n, b, plus_one, which):
    top = 1 << (b - 1)
    parts = []
    for word, ln, flips in _SPECS[which]:
        seg = np.tile(np.array(word, dtype=np.uint8), ln // len(word) + 1)[:ln].copy()
        seg[list(flips)] ^= top
        parts.append(seg)
    t = np.concatenate(parts)
    assert t.size == n and not plus_one and np.isin(t, alphabet(b, plus_one)).all()
    return t


_KINDS = {'mixed': _mixed, 'runs': _runs, 'sprinkled': _sprinkled, 'spec': _spec}

# (kind, seed) per case and size: found by trying seeds until census_ok() had nothing to report.  These are conditions on
# the INPUTS, worked out with the model alone; tests/test_lsd_texts.py asserts them for every entry.
_M, _R, _S = 'mixed', 'runs', 'sprinkled'
PLANTED = {
    (2, 16, 0, 0): ((_M, 66), (_M, 66), (_M, 1), (_M, 1)),
    (2, 16, 1, 0): ((_M, 66), (_M, 66), (_M, 1), (_M, 1)),
    (3, 16, 2, 0): ((_M, 21), (_M, 19), (_M, 4), (_M, 4)),
    (4, 16, 3, 0): ((_M, 4), (_M, 0), (_M, 0), (_M, 0)),
    (5, 12, 4, 0): ((_M, 0), (_M, 7), (_M, 0), (_M, 14)),
    (6, 10, 5, 0): ((_M, 6), (_M, 6), (_M, 6), (_M, 6)),
    (7, 9, 6, 0): ((_M, 8), (_M, 31), (_M, 31), (_M, 38)),
    (8, 8, 0, 0): ((_M, 0), (_M, 0), (_M, 0), (_M, 0)),
    (8, 8, 7, 0): ((_M, 0), (_M, 42), (_M, 92), (_M, 26)),
    (9, 7, 0, 1): ((_M, 8), (_M, 28), (_M, 28), (_M, 8)),
    (9, 7, 8, 1): ((_M, 8), (_M, 28), (_M, 28), (_M, 31)),
    (9, 2, 0, 1): ((_R, 3296), (_R, 4963), (_R, 273), (_R, 466)),
    (8, 2, 7, 0): ((_R, 2846), (_R, 24120), (_S, 4566), (_S, 530)),
    (2, 5, 1, 0): (('spec', 0), ('spec', 1), (_R, 3403), ('spec', 2)),
}


def planted(cfg, n):
    """The planted text of a case (code_bits, key_chars, drop, plus_one) at one of PLANTED_NS."""
    kind, seed = PLANTED[cfg][PLANTED_NS.index(n)]
    return _KINDS[kind](n, cfg[0], cfg[3], seed)


def skewed(n, b, plus_one, seed=6):
    """A text of the `mixed` kind at any size (the case at the cap every build uses)."""
    return _mixed(n, b, plus_one, seed)


# ---- the end of the text --------------------------------------------------------------------------------------------

TAIL_REACH = (0, 1, 7, 8, 15, 16)
TAIL_NS = (12336, 12337, 12351)                  # n mod 16 = 0, 1, 15; four tiles, the last one partial
TAIL_CONFIGS = ((4, 16, 0, 0), (2, 16, 1, 0), (9, 7, 0, 1))
TAIL_COPIES = 5


def tail_case(n, cfg, reach):
    """Random text over three symbols with TAIL_COPIES copies of a word of key_chars symbols planted in it -- a group of
    suffixes tied on the whole key -- and the word's first key_chars - reach symbols as the last symbols of the text: the key
    of that suffix goes on for `reach` symbols past the end, the zero padding is part of it (so it is NOT tied with the
    copies unless reach is 0, and sorts right in front of them: zero is below every symbol).  The suffixes inside that
    last copy reach further still.  reach == key_chars leaves nothing of the word: the text just ends."""
    b, k, _, plus_one = cfg
    assert 0 <= reach <= k
    rng = np.random.default_rng([n, b, k, reach])
    a = alphabet(b, plus_one)
    pick = a[rng.choice(a.size, 3, replace=False)]
    t = pick[rng.integers(0, 3, n)].astype(np.uint8)
    word = pick[rng.integers(0, 3, k)].astype(np.uint8)
    for at in rng.choice(np.arange(64, n - 4 * k, 2 * k), TAIL_COPIES, replace=False):
        t[at:at + k] = word
    if k - reach:
        t[n - (k - reach):] = word[:k - reach]
    return t, word
