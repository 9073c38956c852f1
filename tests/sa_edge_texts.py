"""Texts that put the builder's kernels exactly on their limits (tests/test_sa_edges_gpu.py), and the numpy models
those tests compare the build's statistics with.  Everything here runs on the CPU; tests/test_sa_edge_texts.py runs
every generator for every size the GPU tests use.

planted()  uniform random text with one word written at k places: every position inside the word is a group of exactly
           k tied suffixes; with `lead` (a byte that occurs nowhere else, written before every copy) the joint bucket of
           the suffixes that start at `lead` holds exactly k suffixes.
headed()   uniform random text with several short heads, each written a given number of times: heads that start with
           the same unique byte and differ in their last symbol fill ADJACENT joint buckets with exactly those sizes.
joint_buckets() / tile_heads()   restatements of the joint bucket number of a suffix (text_keys.h: symbols recoded
           densely to 1 .. sigma, packed big-endian, zero past the end; the bucket is the top 20 bits of the key) and of
           the rule that packs consecutive buckets into local-sort tiles (msd_sort.hip, msd_tile_head)."""
import numpy as np

# the constants of msd_sort.hip and sa_rounds_impl.h the cases are built around
MSD_MAX_BUCKET = 4088
MSD_TILE_CAP = 8176
MSD_WIN = 6144
MSD_RAW_TAG_SPAN = 64
MSD_TAG_SPAN = 2048
LS_KMAX = 64
GS_CAP = 512
MID_CAP = 4096

NL = 10
FILL39 = b'abcdefghijklmnopqrstuvwxyz0123456789 .,'            # 39 symbols (+ the final newline: 6-bit codes)
FILL100 = bytes(range(33, 133))                                  # 100 symbols: 7-bit codes
LOWER = b'abcdefghijklmnopqrstuvwxyz'
UPPER = b'ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789'                 # the words of the bucket cases: no symbol of the fill
FILL70 = bytes(range(48, 118))                                   # 70 symbols: 7-bit codes, 3 symbols cover 20 bits
LEAD = 0xF5                                                      # larger than every other byte: its buckets end the suffix array

BUCKET_KS = (4087, 4088, 4089, 4090, 8176, 8177)
BIN_KS = (2, 7, 8, 9, 16, 63, 64, 65, 66, 200)
TAIL_DS = (0, 1, 7, 8, 15, 16)
MID_KMAX = 512
TIER_KS = (GS_CAP - 1, GS_CAP, GS_CAP + 1, MID_CAP - 1, MID_CAP, MID_CAP + 1, 8191, 8192, 8193)      # (8193 = 2 * 4096 + 1)


def _fill(rng, alphabet, count):
    a = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    return a[rng.integers(0, len(a), count)]


def _continuations(rng, alphabet, k):
    """k different strings of equal length over the alphabet, in random order."""
    a = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    digits = 3
    while len(a) ** digits < 4 * k:
        digits += 1
    ids = rng.choice(len(a) ** digits, size=k, replace=False)
    out = np.empty((k, digits), np.uint8)
    for d in range(digits):
        out[:, d] = a[ids % len(a)]
        ids = ids // len(a)
    return out


def _assemble(rng, n, alphabet, units, last_gap=None):
    """The units in the given order, random fill between them, a newline at the end: n bytes."""
    t = np.empty(n, np.uint8)
    t[:n - 1] = _fill(rng, alphabet, n - 1)                  # (drawn first: the same fill whatever is planted)
    total = sum(len(u) for u in units)
    room = n - 1 - total
    assert room >= 0, (n, total)
    slots = len(units) + 1
    if last_gap is not None:
        assert room >= last_gap
        gaps = np.append(rng.multinomial(room - last_gap, np.full(slots - 1, 1.0 / (slots - 1))), last_gap)
    else:
        gaps = rng.multinomial(room, np.full(slots, 1.0 / slots))
    at = 0
    for u, g in zip(units, gaps[:-1]):
        at += int(g)
        t[at:at + len(u)] = u
        at += len(u)
    assert at + int(gaps[-1]) == n - 1
    t[n - 1] = NL
    return t


def make_word(rng, symbols, length, gram=3):
    """A random word all of whose windows of `gram` symbols are different: it has no period, and no two of its positions
    share their first `gram` symbols (gram = 2: nor a joint bucket, whatever the code width -- 20 bits hold two symbols)."""
    a = np.frombuffer(bytes(symbols), dtype=np.uint8)
    while True:
        w = a[rng.integers(0, len(a), length)]
        grams = {bytes(w[i:i + gram]) for i in range(length - gram + 1)}
        if len(grams) == length - gram + 1:
            return bytes(w)


def count_sharing(t, piece):
    """Suffixes of t that start with `piece` (overlapping occurrences count)."""
    t = np.ascontiguousarray(t)
    p = np.frombuffer(bytes(piece), dtype=np.uint8)
    if len(p) > t.size:
        return 0
    hit = t[:t.size - len(p) + 1] == p[0]
    cand = np.flatnonzero(hit)
    for j in range(1, len(p)):
        if cand.size == 0:
            break
        cand = cand[t[cand + j] == p[j]]
    return int(cand.size)


def planted(rng, n, alphabet, word, k, lead=None, *, tail=None, second=None, same=0):
    """Uniform random text over `alphabet` (which has neither the newline nor `lead`), n bytes, ending in a newline, with
    `word` at k non-overlapping places.  Every copy goes on differently (a continuation no other copy has), so the k
    suffixes at one position of the word are tied exactly as far as the word goes.
      lead    a byte written before every copy and nowhere else
      tail    the copy that comes last in the text ends this many bytes before the final newline
      second  a second word that follows the first in k // 2 of the copies (the group splits into one of k // 2 and singletons)
      same    all copies but three go on with this many times the alphabet's first byte before their own continuation (one
              round sees k - 3 equal keys and 3 others)
    The construction is checked before the text is returned: `word` and `lead` occur k times, and at three offsets of the
    word exactly k suffixes share the rest of it."""
    word = bytes(word)
    assert 80 <= len(word) <= 300 and k >= 2
    assert NL not in alphabet and NL not in word and (lead is None or (lead not in alphabet and lead not in word))
    cont = _continuations(rng, alphabet, k)
    head = bytes([lead]) if lead is not None else b''
    run = bytes([alphabet[0]]) * same
    if same:
        # the three copies without the run go on with another byte than the run's: their keys leave the others' bin at once
        other = np.flatnonzero(cont[:, 0] != alphabet[0])[:3]
        rest = np.setdiff1d(np.arange(k), other)
        cont = cont[np.concatenate([other, rest])]
    units = []
    for i in range(k):
        u = head + word
        if second is not None and i < k // 2:
            u += bytes(second)
        if same and i >= 3:
            u += run
        units.append(np.frombuffer(u + bytes(cont[i]), dtype=np.uint8))
    order = rng.permutation(k)
    units = [units[i] for i in order]
    last_gap = None
    if tail is not None:
        last = units[-1]
        keep = len(head) + len(word)
        units[-1] = last[:keep + min(tail, len(last) - keep)]
        last_gap = tail - (len(units[-1]) - keep)
    t = _assemble(rng, n, alphabet, units, last_gap)
    check_planted(t, word, k, lead, second)
    if tail is not None:
        assert bytes(t[n - 1 - tail - len(word):n - 1 - tail]) == word
    return t


def check_planted(t, word, k, lead=None, second=None):
    assert t[-1] == NL
    L = len(word)
    assert count_sharing(t, word) == k, ('word', count_sharing(t, word), k)
    if lead is not None:
        assert int(np.count_nonzero(t == lead)) == k, ('lead', int(np.count_nonzero(t == lead)), k)
    for off in (1, L // 3, (2 * L) // 3):
        got = count_sharing(t, word[off:])
        assert got == k, ('offset', off, got, k)
    if second is not None:
        assert count_sharing(t, word + bytes(second)) == k // 2
    # (no run-length path, no closed form: the text is random between the copies and no copy goes on like another)
    runs = 1 + int(np.count_nonzero(t[1:] != t[:-1]))
    assert runs * 8 > t.size


def headed(rng, n, alphabet, heads, sizes):
    """Uniform random text over `alphabet` with heads[g] written sizes[g] times, random text behind every copy.  Every head
    starts with a byte that is not in the alphabet, so nothing else shares a head's first symbols."""
    units = []
    for h, c in zip(heads, sizes):
        assert h[0] not in alphabet and NL not in alphabet
        units += [np.frombuffer(bytes(h), dtype=np.uint8)] * c
    units = [units[i] for i in rng.permutation(len(units))]
    t = _assemble(rng, n, alphabet, units)
    firsts = {h[0] for h in heads}
    assert int(np.isin(t, list(firsts)).sum()) == sum(sizes)
    for h, c in zip(heads, sizes):
        assert count_sharing(t, h) == c, (h, count_sharing(t, h), c)
    return t


# ---- models ----------------------------------------------------------------------------------------------------------

def code_bits_of(t):
    sigma = int(np.unique(t).size)
    assert sigma < 256
    return sigma.bit_length()                    # codes 0 .. sigma


def joint_buckets(t, code_bits=None, key_chars=None, key_bits=None):
    """Joint bucket number of every suffix: bytes -> dense codes 1 .. sigma in byte order (0 past the end of the text),
    key_chars codes packed big-endian, code_bits each; the sort key is that number without its lowest
    key_chars * code_bits - key_bits bits; the bucket is the key's top 20 bits.  Without the three arguments: as many
    symbols as cover 20 bits (the top 20 bits do not depend on how long the key is)."""
    t = np.ascontiguousarray(t, dtype=np.uint8)
    present = np.unique(t)
    b = code_bits_of(t)
    if code_bits is not None:
        assert int(code_bits) == b, (code_bits, b)
    kc = int(key_chars) if key_chars else (20 + b - 1) // b
    kb = int(key_bits) if key_bits else kc * b
    assert 20 <= kb <= kc * b <= 64
    lut = np.zeros(256, np.uint64)
    lut[present] = np.arange(1, present.size + 1, dtype=np.uint64)
    codes = np.concatenate([lut[t], np.zeros(kc, np.uint64)])
    key = np.zeros(t.size, np.uint64)
    for j in range(kc):
        key = (key << np.uint64(b)) | codes[j:j + t.size]
    key >>= np.uint64(kc * b - kb)
    return (key >> np.uint64(kb - 20)).astype(np.int64)


def bucket_sizes(t):
    """(joint bucket numbers of the non-empty buckets, their sizes), in bucket order."""
    j, c = np.unique(joint_buckets(t), return_counts=True)
    return j, c


def lsd_numbers(numbers):
    """The number a joint bucket goes by in LSD order: [first digit | second digit], the second digit renumbered among the
    digit values that occur in the text at all (msd_tiles2_kernel: a value that never occurs leaves no hole)."""
    numbers = np.asarray(numbers, dtype=np.int64)
    d = numbers & 1023
    return (numbers >> 10 << 10) | np.searchsorted(np.unique(d), d)


def tile_heads(numbers, sizes, n, lsd=True):
    """Which non-empty buckets start a local-sort tile (msd_tile_head): the buckets whose first slot falls into one
    window of MSD_WIN slots share a tile; when the window's buckets hold more than MSD_TILE_CAP elements together its last
    bucket goes alone; and a tile never crosses an aligned block of 64 joint buckets (LSD order, the default) or of 2048
    non-empty ones (PSS_MSD_LSD=0)."""
    ne = len(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert start[-1] == n
    cs = start[:-1]
    k = np.arange(ne)
    block = (lsd_numbers(numbers) // MSD_RAW_TAG_SPAN) if lsd else (k // MSD_TAG_SPAN)
    w = cs // MSD_WIN
    head = np.zeros(ne, bool)
    head[0] = True
    head[1:] |= block[1:] != block[:-1]
    head[1:] |= w[1:] != w[:-1]
    last = np.ones(ne, bool)
    last[:-1] = w[1:] != w[:-1]
    first_of_window = np.searchsorted(cs, w * MSD_WIN, side='left')
    over = start[1:] - cs[first_of_window] > MSD_TILE_CAP
    head |= last & over
    return head


def tile_count(t, lsd=True):
    numbers, sizes = bucket_sizes(t)
    return int(tile_heads(numbers, sizes, t.size, lsd).sum())


# ---- the cases -------------------------------------------------------------------------------------------------------

def bucket_case(k):
    """planted() with a lead byte: the joint bucket of the suffixes that start at the lead holds exactly k, every position
    of the word another k, and no other bucket comes near (the word has no symbol of the fill; its 2-symbol windows are
    all different)."""
    rng = np.random.default_rng(1000 + k)
    word = make_word(rng, UPPER, 80, gram=2)
    n = (1 << 19) + 37 if k < 5000 else (1 << 20) - 11
    t = planted(rng, n, LOWER, word, k, lead=LEAD)
    numbers, sizes = bucket_sizes(t)
    assert int(sizes.max()) == k, (int(sizes.max()), k)
    lead_bucket = joint_buckets(t)[np.flatnonzero(t == LEAD)]
    assert np.unique(lead_bucket).size == 1 and sizes[np.searchsorted(numbers, lead_bucket[0])] == k
    return t


def _head(s1, s2):
    return bytes([LEAD, s1, s2])


def _codes70():
    """byte -> code in the texts of headed() over FILL70 (newline = 1, the fill 2 .. 71, the lead 72: 7 bits)."""
    present = sorted(set(FILL70) | {NL, LEAD})
    return {c: i + 1 for i, c in enumerate(present)}


def tile_case(name):
    """Large buckets next to each other INSIDE one aligned block of 64 joint buckets: heads lead + s1 + s2 -- with 7-bit
    codes the joint bucket is [lead | s1 | s2 >> 1], so heads that differ in s2 only are neighbours (bucket number mod 64 =
    code(s2) >> 1) and nothing else starts with the lead.  The lead is the largest byte: its buckets are the last of the
    suffix array and the text's length puts their first slot where the case wants it in the MSD_WIN grid.
      pair8176   4088 + 4088 from the start of a window: one tile (exactly MSD_TILE_CAP)
      trio8177   1 + 4088 + 4088 from the start of a window: 8177, the last bucket goes alone
      run        2000 + 2000 + 2000 + 4000, all starting inside one window: 10000, the last bucket goes alone
      chain      4088 after 4088 after 4088, not aligned: every bucket first of its window"""
    sizes, offset = {'pair8176': ((4088, 4088), 0), 'trio8177': ((1, 4088, 4088), 0),
                     'run': ((2000, 2000, 2000, 4000), 0), 'chain': ((4088, 4088, 4088), 3000)}[name]
    code = _codes70()
    s2 = [c for c in FILL70 if code[c] % 2 == 0][:len(sizes)]          # codes 2, 4, 6, ...: buckets 1, 2, 3 of the block
    heads = [_head(FILL70[40], c) for c in s2]
    total = sum(sizes)
    n = MSD_WIN * 40 + offset + total                                  # the lead's first bucket starts at 40 windows + offset
    # (the pair and the trio share everything but one head: the seed is looked for once, see tile_pair_seed)
    rng = np.random.default_rng(_TILE_SEEDS.get(name, 77))
    t = headed(rng, n, FILL70, heads, sizes)
    assert code_bits_of(t) == 7
    numbers, got = bucket_sizes(t)
    assert tuple(got[-len(sizes):]) == tuple(sizes) and int(got[:-len(sizes)].max()) < 1000
    assert np.unique(lsd_numbers(numbers)[-len(sizes):] // 64).size == 1
    assert (t.size - total) % MSD_WIN == offset
    return t


_TILE_SEEDS = {'pair8176': 79, 'trio8177': 79}      # (a fill with which the rest of the text plans equally many tiles in both)


def _slotted(n, heads, sizes, seed, pitch=24):
    """The same random text over FILL70 whatever is planted; copy number i of the heads (in the order given) at byte
    24 i + 8: one head more changes three bytes and nothing else."""
    rng = np.random.default_rng(seed)
    t = np.empty(n, np.uint8)
    t[:n - 1] = _fill(rng, FILL70, n - 1)
    t[n - 1] = NL
    at = 8
    for h, c in zip(heads, sizes):
        for _ in range(c):
            t[at:at + len(h)] = np.frombuffer(bytes(h), dtype=np.uint8)
            at += pitch
    assert at < n - 8
    for h, c in zip(heads, sizes):
        assert count_sharing(t, h) == c
    assert int(np.count_nonzero(t == LEAD)) == sum(sizes)
    return t


def tagblock_case(big, lsd):
    """Random text over 70 symbols, 2^17 bytes: 170 000 possible joint buckets for 131 072 suffixes -- every non-empty
    bucket tiny, thousands of them in a row inside one MSD_WIN window, so the tiles are cut by the tag blocks alone (64
    joint buckets in LSD order, 2048 non-empty ones with PSS_MSD_LSD=0).  big: one bucket of 3000 sitting exactly on a
    block boundary -- LSD order: head lead + s1 + newline with code(s1) = 16 (second digit 0: number = 0 mod 64); MSD order: single-element
    spacer heads before it, as many as bring its number among the non-empty buckets to a multiple of 2048."""
    n = (1 << 17) + 5
    if not big:
        t = _slotted(n, [_head(FILL70[3], FILL70[3])], [1], 5)
    elif lsd:
        t = _slotted(n, [_head(FILL70[14], NL)], [3000], 6)              # (code 16, newline: second digit 0)
        numbers, sizes = bucket_sizes(t)
        assert sizes[-1] == 3000 and lsd_numbers(numbers)[-1] % MSD_RAW_TAG_SPAN == 0
    else:
        code = _codes70()
        spare = [_head(a, c) for a in FILL70[:69] for c in FILL70 if code[c] % 2 == 0]      # distinct buckets before the big one
        # (a spacer adds its own bucket and takes some of its neighbours' away; this choice was looked for once -- the text
        # is the same on every machine -- and the check below holds it to the boundary)
        heads = spare[:1423] + spare[2000:2005]
        t = _slotted(n, [_head(FILL70[69], FILL70[0])] + heads, [3000] + [1] * len(heads), 7)
        sizes = bucket_sizes(t)[1]
        assert sizes[-1] == 3000 and (len(sizes) - 1) % MSD_TAG_SPAN == 0, len(sizes)
    numbers, sizes = bucket_sizes(t)
    assert int(np.sort(sizes)[-2 if big else -1]) <= 200 and code_bits_of(t) == 7      # (200: the suffixes one byte into the big bucket's head)
    return t


def bin_case(k, wide=False):
    """planted() without a lead: every position of the word is k equal keys in one bin of the local sort."""
    rng = np.random.default_rng(2000 + k + (500 if wide else 0))
    alphabet = FILL100 if wide else FILL39
    word = make_word(rng, alphabet, 90)
    return planted(rng, (1 << 17) + 3 + k % 7, alphabet, word, k)


def tail_case(d):
    rng = np.random.default_rng(3000 + d)
    word = make_word(rng, FILL39, 90)
    n = (1 << 17) + 1 + 2 * d                      # 131073 .. 131105: never a multiple of 16
    assert n % 16
    return planted(rng, n, FILL39, word, 70, tail=d)


def tier_case(k, variant='plain'):
    """Groups of exactly k in the rounds: a word of 240 symbols (200 from k = 4095 on, 90 from k = 8191 on: 8193 copies of more
    do not fit 2^20 bytes).  second: half of the copies share 40 more symbols; crowded: all but three go on with 5 equal bytes --
    fewer than the initial key packs (6 symbols of 6 bits at these sizes), or the suffixes INSIDE those runs would share
    their whole key and form one group of several times k."""
    rng = np.random.default_rng(4000 + k + {'plain': 0, 'second': 100000, 'crowded': 200000}[variant])
    length = 240 if k < 4090 else (200 if k < 5000 else 90)
    word = make_word(rng, FILL39, length)
    extra = {}
    if variant == 'second':
        extra['second'] = make_word(rng, FILL39, 80)[:40]
    elif variant == 'crowded':
        extra['same'] = 5
    per = length + 4 + (20 if variant == 'second' else 0) + (5 if variant == 'crowded' else 0)
    n = max(1 << 17, min((1 << 20) - 5, k * per + (1 << 14)))
    return planted(rng, n + (1 - n % 2), FILL39, word, k, **extra)


def switch_planted():
    rng = np.random.default_rng(600)
    return planted(rng, (1 << 19) + 9, FILL39, make_word(rng, FILL39, 200), 600)
