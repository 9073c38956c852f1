"""A CPU model of the rounds (pysubstringsearch_amd/csrc/sa_refine_impl.h driving sa_rounds_impl.h and sa_rerank_impl.h),
and the texts that put each of its decisions on its edge (tests/test_rounds_gpu.py compares a build's statistics with
walk() for equality; tests/test_rounds_model.py holds walk() itself to a brute force, on the CPU).

walk()   which rounds a build makes -- kind, depth, length of the active list, members of the large groups, whether a
         text round gave up -- and the totals the build reports: rounds, text_rounds, sum_active, big_elems, mode.
         Two restatements, and nothing else:
           the classes   a suffix's rank is 1 + the SA slot of the head of its group (rr_apply_kernel).  A text round
                         splits every group by the next kt symbols (text_keys_kernel), a rank or global round by the rank
                         of suffix i + h (rank_keys_kernel, build_keys_kernel): the classes after the round are the
                         distinct pairs (rank, new key), found with np.unique on packed 64-bit pairs.  A suffix is on
                         the active list iff its group has more than one member.
           the driver    Rounds::run, in its order, with the rules of rounds_layout.h restated below.
         Out of the model: the anchor round, periodic keys, the run-length path and the closed form, the MSD finishing
         kernel.  A build is comparable when they are switched off (EXACT).
CASES    the texts, generators with fixed seeds; every generator asserts that its text sits where the case says.
EDGES    pairs of cases on the two sides of one decision: their walks must differ in a total a build reports."""
from collections import namedtuple

import numpy as np

from tests import sa_edge_texts as E

GS_CAP, MID_CAP, MID_KMAX = E.GS_CAP, E.MID_CAP, E.MID_KMAX
MID_BINS = 4096                                   # sa_rounds_impl.h: bins of mid_sort_kernel
M_DENSE, M_SPARSE, M_TEXT = 0, 1, 2               # rounds_layout.h: RoundMode
TEXT_ROUNDS_DEFAULT = 5                           # sa_plan_impl.h: Knobs::text_rounds_max
MAX_ROUNDS = 96                                   # Rounds::run

# what every exact comparison switches off (the parts the model leaves out) and the initial sort it asks for
EXACT = {'PSS_MSD': '0', 'PSS_SS': '0', 'PSS_RLE': '0', 'PSS_PERIOD': '0', 'PSS_ANCHOR': '0', 'PSS_PERIODIC': '0'}
TOTALS = ('rounds', 'text_rounds', 'sum_active', 'big_elems', 'mode')

Round = namedtuple('Round', 'kind h m nbig gave_up')


class Walk:
    def __init__(self):
        self.rounds_list = []
        self.rounds = self.text_rounds = self.sum_active = self.big_elems = 0
        self.mode = 0
        self.m0 = 0                # suffixes the initial sort left tied
        self.h0 = 0
        self.h_final = 0           # symbols every group is known to share when nothing is tied any more
        self.first_mode = 0
        self.classes = []          # keep_classes: (depth, rank of every suffix) before the first round and after each

    def totals(self):
        return tuple(int(getattr(self, k)) for k in TOTALS)

    def __str__(self):
        lines = ['rounds=%d text_rounds=%d sum_active=%d big_elems=%d mode=%d (m0=%d h0=%d)' % (self.totals() + (self.m0, self.h0))]
        lines += ['  %-6s h=%-6d m=%-8d nbig=%-8d%s' % (r.kind, r.h, r.m, r.nbig, ' gave up' if r.gave_up else '') for r in self.rounds_list]
        return '\n'.join(lines)


# ---- the rules of rounds_layout.h --------------------------------------------------------------------------------------

def symbols_per_key(b):
    return min(16, 64 // b)


def first_mode(n, m_next, knob_mode, text_rounds_max, rank_only):
    mode = M_SPARSE if m_next * 1024 <= n else M_TEXT
    if knob_mode >= 0:
        mode = knob_mode
    if mode == M_SPARSE and m_next * 16 > n:
        mode = M_TEXT
    if m_next == 0:
        mode = M_SPARSE
    if mode == M_TEXT and text_rounds_max <= 0:
        mode = M_DENSE
    if rank_only and m_next:
        mode = M_DENSE
    return mode


def text_round_gives_up(nbig, m, text_rounds):
    return nbig * 2 > m and (text_rounds > 0 or nbig * 4 > m * 3)


def text_progress(m, m_text_prev, text_rounds):
    return text_rounds == 0 or m * 10 <= m_text_prev * 6


def goes_global(last_big_frac, last_per, m):
    return m // 2 if last_big_frac > 0.5 and not last_per else 0


def knobs_of(switches):
    """The switches the walk depends on (sa_plan_impl.h: Knobs::read).  The rest choose kernels, not rounds."""
    mode = {None: -1, 'dense': M_DENSE, 'sparse': M_SPARSE, 'text': M_TEXT}[switches.get('PSS_MODE')]
    return dict(mode=mode, text_rounds_max=int(switches.get('PSS_TEXT_ROUNDS', TEXT_ROUNDS_DEFAULT)),
                no_mid_tier='PSS_NO_MID_TIER' in switches, no_mid_merge='PSS_NO_MID_MERGE' in switches)


def walk_key(switches):
    """Two sets of switches with the same walk_key must give the same walk."""
    return tuple(sorted(knobs_of(switches).items()))


# ---- the classes -------------------------------------------------------------------------------------------------------

def recode(text):
    """Dense codes 1 .. sigma in symbol order (choose_codes; the reduced string of the run-length path: any integers)."""
    text = np.ascontiguousarray(text)
    present, inv = np.unique(text, return_inverse=True)
    return (inv.reshape(-1) + 1).astype(np.uint64), int(present.size)


def pack(padded, start, count, k, b):
    """Keys of k symbols of b bits, big-endian, for the positions start .. start + count of the zero-padded codes."""
    key = np.zeros(count, np.uint64)
    for j in range(k):
        key = (key << np.uint64(b)) | padded[start + j:start + j + count]
    return key


def ranks_of(keys):
    """(rank, group size) of every element of a list that is sorted by `keys`: rank = 1 + slot of the group's head."""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    head = np.cumsum(cnt) - cnt
    return (head[inv] + 1).astype(np.int64), cnt[inv].astype(np.int64)


def _crowded(rank, size, act, newkey):
    """Members of the groups of GS_CAP + 1 .. MID_CAP suffixes that mid_sort_kernel hands on: it bins the members on the
    12 bits below the highest bit in which their keys differ, and gives up when a bin holds more than MID_KMAX of them
    (a group whose keys are all equal is in order as it stands)."""
    pick = (size[act] > GS_CAP) & (size[act] <= MID_CAP)
    if not pick.any():
        return 0
    g, k = rank[act][pick], newkey[pick]
    order = np.argsort(g, kind='stable')
    g, k = g[order], k[order]
    starts = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    lens = np.diff(np.concatenate([starts, [g.size]]))
    diff = np.bitwise_or.reduceat(k ^ np.repeat(k[starts], lens), starts)
    shift = np.array([max(int(d).bit_length() - 12, 0) for d in diff], np.uint64)
    bins = (k >> np.repeat(shift, lens)) & np.uint64(MID_BINS - 1)
    which = np.repeat(np.arange(starts.size), lens)
    fullest = np.bincount(which * MID_BINS + bins.astype(np.int64), minlength=starts.size * MID_BINS).reshape(-1, MID_BINS).max(axis=1)
    return int(lens[(diff != 0) & (fullest > MID_KMAX)].sum())


def walk(text, *, key_chars, key_bits, code_bits, switches, rank_only=False, keep_classes=False):
    """The rounds of a build of `text` whose initial sort took the top key_bits bits of key_chars symbols of code_bits
    bits.  rank_only: the text is a string of integers, one symbol per key, rank rounds from depth 1 (the reduced string
    of the run-length path)."""
    kn = knobs_of(switches)
    codes, sigma = recode(text)
    n = int(codes.size)
    b = int(code_bits)
    assert n >= 2
    w = Walk()
    if rank_only:
        assert key_chars == 1
        kt, h = 0, 1
        rank, size = ranks_of(codes)
        padded = None
    else:
        assert sigma < (1 << b) and 1 <= key_chars and key_bits <= key_chars * b <= 64 and key_bits > (key_chars - 1) * b
        kt = symbols_per_key(b)
        padded = np.concatenate([codes, np.zeros(max(kt, key_chars) + 1, np.uint64)])
        rank, size = ranks_of(pack(padded, 0, n, key_chars, b) >> np.uint64(key_chars * b - key_bits))
        h = key_chars if key_bits == key_chars * b else key_chars - 1
    w.h0 = h
    w.m0 = int((size > 1).sum())
    mode = first_mode(n, w.m0, kn['mode'], kn['text_rounds_max'], rank_only)
    w.first_mode = mode
    was_text = mode == M_TEXT
    text_rounds = m_text_prev = global_above = 0
    limit = GS_CAP if kn['no_mid_tier'] else MID_CAP
    if keep_classes:
        w.classes.append((h, rank.copy()))

    def new_keys(act, use_text):
        if use_text:
            at = np.minimum(act + h, n)                    # (past the end: zeros, text_keys_kernel)
            key = np.zeros(act.size, np.uint64)
            for j in range(kt):
                key = (key << np.uint64(b)) | padded[np.minimum(at + j, n)]
            return key
        nxt = act + h
        return np.where(nxt < n, rank[np.minimum(nxt, n - 1)], 0).astype(np.uint64)

    def refine(act, key):
        """The groups split by the new key; the members of a group keep its slots."""
        dense = np.unique(key, return_inverse=True)[1].reshape(-1).astype(np.uint64) if key.size and int(key.max()) >> 32 else key
        pair = (rank[act].astype(np.uint64) << np.uint64(32)) | dense
        u, inv, cnt = np.unique(pair, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        slot = np.cumsum(cnt) - cnt                        # first slot of every new group among the active
        grp = (u >> np.uint64(32)).astype(np.int64)
        first = np.concatenate([[True], grp[1:] != grp[:-1]])
        base = np.maximum.accumulate(np.where(first, slot, 0))
        rank[act] = grp[inv] + (slot - base)[inv]
        size[act] = cnt[inv]

    for _ in range(MAX_ROUNDS + 1):
        act = np.flatnonzero(size > 1)
        m = int(act.size)
        if m == 0:
            break
        assert h < n, 'suffixes unresolved at h >= n'
        took = False
        if mode == M_TEXT:
            bail = True
            if text_rounds < kn['text_rounds_max'] and text_progress(m, m_text_prev, text_rounds):
                m_text_prev = m
                key = new_keys(act, True)
                nbig = int((size[act] > limit).sum())
                if kn['no_mid_merge'] and not kn['no_mid_tier']:
                    nbig += _crowded(rank, size, act, key)
                bail = nbig > 0 and text_round_gives_up(nbig, m, text_rounds)
                w.rounds_list.append(Round('text', h, m, nbig, bail))
                if not bail:
                    refine(act, key)
                    text_rounds += 1
                    h += kt
                    took = True
            if bail:
                mode = M_DENSE
        if not took and mode == M_DENSE:
            if m <= global_above:
                global_above = 0
            if global_above == 0:
                key = new_keys(act, False)
                nbig = int((size[act] > limit).sum())
                if kn['no_mid_merge'] and not kn['no_mid_tier']:
                    nbig += _crowded(rank, size, act, key)
                w.rounds_list.append(Round('rank', h, m, nbig, False))
                refine(act, key)
                global_above = goes_global(nbig / m, False, m)
                h *= 2
                took = True
        if not took:
            w.rounds_list.append(Round('global', h, m, 0, False))
            refine(act, new_keys(act, False))
            h *= 2
        if keep_classes:
            w.classes.append((h, rank.copy()))
    else:
        raise AssertionError('no convergence')
    done = [r for r in w.rounds_list if not r.gave_up]
    w.rounds = len(done)
    w.text_rounds = sum(r.kind == 'text' for r in done)
    w.sum_active = sum(r.m for r in done)
    w.big_elems = sum(r.nbig for r in done if r.kind != 'global')
    w.mode = (2 if mode == M_TEXT else 3) if was_text else mode
    w.h_final = h
    return w


# ---- the texts ---------------------------------------------------------------------------------------------------------
# A family is one random word written `copies` times.  Up to len(alphabet) copies go on, and are preceded, by a different
# symbol each: at offset p of the word exactly `copies` suffixes share exactly length - p symbols.  More copies than that
# carry a number unique to the copy, in three digits before the word (least significant digit next to the word) and
# behind it: how the suffixes around the word are tied is then the same whatever lies between the copies.

def _units(rng, alphabet, length, copies):
    a = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    word = a[rng.integers(0, a.size, length)]
    A = a.size
    out = []
    if copies <= A:
        pre, post = rng.permutation(A)[:copies], rng.permutation(A)[:copies]
        for i in range(copies):
            out.append(np.concatenate([[a[pre[i]]], word, [a[post[i]]]]).astype(np.uint8))
    else:
        assert copies <= A ** 3
        ids = rng.permutation(copies)
        for i in ids:
            d = np.array([i % A, i // A % A, i // A // A])
            out.append(np.concatenate([a[d[::-1]], word, a[d]]).astype(np.uint8))
    return out


def plant(seed, n, alphabet, families):
    """n bytes: uniform random text over the alphabet, a final newline, and the families' copies at random places."""
    rng = np.random.default_rng(seed)
    units = []
    for length, copies in families:
        units += _units(rng, alphabet, length, copies)
    units = [units[i] for i in rng.permutation(len(units))]
    return E._assemble(rng, n, alphabet, units)


def params_of(t, key_chars):
    b = E.code_bits_of(t)
    return dict(key_chars=key_chars, key_bits=key_chars * b, code_bits=b)


class Case:
    """make() -> text; key_chars: PSS_KEY_CHARS of the build; switches: the case's own (EXACT comes on top); small(): the
    same families in a text of 2^12 bytes, where they fit (the brute force of tests/test_rounds_model.py)."""
    def __init__(self, make, key_chars, switches=None, small=None):
        self.make, self.key_chars, self.switches, self.small = make, key_chars, dict(switches or {}), small
        self._text = self._walk = None

    def text(self):
        if self._text is None:
            t = np.ascontiguousarray(self.make())
            t.setflags(write=False)
            self._text = t
        return self._text

    def env(self):
        return dict(EXACT, PSS_KEY_CHARS=str(self.key_chars), **self.switches)

    def walk(self):
        if self._walk is None:
            self._walk = walk(self.text(), switches=self.switches, **params_of(self.text(), self.key_chars))
        return self._walk


CASES = {}
EDGES = []           # (case, case): the two sides of one decision
N16 = (1 << 16)
SMALL = 1 << 12
K8 = 8               # the key of most cases: 8 symbols of 6 or 7 bits -- random text over 39 symbols has no ties of its own then


def _w(t, key_chars, switches):
    return walk(t, switches=switches, **params_of(t, key_chars))


def _split(total):
    """total = 2 a + 3 c with c in (0, 1): pairs and at most one triple of a word of exactly key_chars symbols."""
    c = total % 2
    assert total >= 3 * c
    return [(K8, 2)] * ((total - 3 * c) // 2) + [(K8, 3)] * c


# -- sparse or text: m0 * 1024 against n, and m0 * 16 against n under PSS_MODE=sparse

def _mode_text(m0, long_word, n=N16):
    """m0 suffixes tied by the initial key and nothing else: one word written twice (long_word: of m0 // 2 tied places,
    else of 30) and words of key_chars symbols written twice or three times for the rest."""
    places = (m0 - 3 * (m0 % 2)) // 2 if long_word else 30
    rest = m0 - 2 * places
    fam = [(K8 + places - 1, 2)] + (_split(rest) if rest else [])
    return plant(100 + m0, n, E.FILL39, fam)


def _mode_case(m0, switches, long_word, want_mode):
    def make():
        t = _mode_text(m0, long_word)
        w = _w(t, K8, switches)
        assert t.size == N16 and w.m0 == m0, (w.m0, m0)
        assert w.first_mode == want_mode, (w.first_mode, want_mode)
        return t
    return Case(make, K8, switches, None if long_word else lambda: _mode_text(m0, long_word, SMALL))


for _m0, _mode in ((63, M_SPARSE), (64, M_SPARSE), (65, M_TEXT)):          # m0 * 1024 = n - 1024, n, n + 1024
    CASES['mode_%d' % _m0] = _mode_case(_m0, {}, False, _mode)
EDGES += [('mode_63', 'mode_64'), ('mode_64', 'mode_65')]
for _m0, _mode in ((4095, M_SPARSE), (4096, M_SPARSE), (4097, M_TEXT)):    # m0 * 16 = n - 16, n, n + 16: the hash table fits or not
    CASES['sparse_%d' % _m0] = _mode_case(_m0, {'PSS_MODE': 'sparse'}, True, _mode)
EDGES += [('sparse_4095', 'sparse_4096'), ('sparse_4096', 'sparse_4097')]


# -- depth bookkeeping: one word written twice whose copies part in text round j (depth h0 + j kt) or rank round j (h0 2^j)

def _decoys(main, h0, kt, rounds):
    """Words written twice that text round r = 1 .. rounds - 1 resolves, as many as keep every text round up to `rounds`
    worth running (text_progress: a round starts only with at most 6/10 of the list its predecessor started with)."""
    count = {}
    def tied(s):          # members of the list that text round s + 1 starts with
        total = 2 * max(main - (h0 + s * kt) + 1, 0)
        for r, c in count.items():
            total += 2 * c * max((r - 1 - s) * kt + 1, 0)
        return total
    for s in range(rounds - 2, -1, -1):
        count[s + 1] = 0
        while tied(s + 1) * 10 > tied(s) * 6 - 12:
            count[s + 1] += 1
    return [(h0 + (r - 1) * kt, 2) for r, c in sorted(count.items()) for _ in range(c)]


def _depth_case(alphabet, kt, j, d, dense):
    """The copies share exactly L = edge + d symbols, edge = h0 + j kt (text rounds) or h0 2^j (rank rounds): with d = -1
    round j parts them, with d = 0 or 1 it takes one more."""
    h0 = K8
    L = (h0 << j if dense else h0 + j * kt) + d
    switches = {'PSS_MODE': 'dense' if dense else 'text'}
    want = j + (1 if d >= 0 else 0)

    def text(n):
        fam = [(L, 2)] + ([] if dense else _decoys(L, h0, kt, want))
        return plant(200 + 16 * j + d + (64 if dense else 0) + len(alphabet), n, alphabet, fam)

    def make():
        t = text(N16 + 2 * j + 1)
        assert symbols_per_key(E.code_bits_of(t)) == kt
        w = _w(t, K8, switches)
        kinds = [r.kind for r in w.rounds_list]
        assert kinds == ['rank' if dense else 'text'] * want, (kinds, want, str(w))
        depths = [r.h for r in w.rounds_list]
        assert depths == [(h0 << i) if dense else h0 + i * kt for i in range(want)], depths
        assert w.rounds_list[-1].m == 2 * (L - depths[-1] + 1), str(w)      # the last round sees the two copies alone
        return t
    return Case(make, K8, switches, lambda: text(SMALL + 1))


for _name, _alpha, _kt in (('b6', E.FILL39, 10), ('b7', E.FILL100, 9)):
    for _j in (1, 2, 3, 4):
        for _dense in (False, True):
            _ids = []
            for _d in (-1, 0, 1):
                _id = '%s_%s_%d_%s' % ('dense' if _dense else 'text', _name, _j, {-1: 'below', 0: 'at', 1: 'above'}[_d])
                CASES[_id] = _depth_case(_alpha, _kt, _j, _d, _dense)
                _ids.append(_id)
            EDGES += [(_ids[0], _ids[1]), (_ids[1], _ids[2])]


def _binary_case(L):
    """Two symbols: 2-bit codes, a text-round key of 16 symbols (not 32).  Random text over two symbols is full of ties of
    its own at 16 symbols, few at 32; the planted copies share L symbols."""
    switches = {'PSS_MODE': 'text'}

    def make():
        t = plant(300, N16 + 5, b'ab', [(L, 2)])
        assert E.code_bits_of(t) == 2 and symbols_per_key(2) == 16
        w = _w(t, 16, switches)
        assert w.rounds_list[0][:2] == ('text', 16) and w.rounds_list[1][:2] == ('text', 32), str(w)
        return t
    return Case(make, 16, switches, lambda: plant(300, SMALL + 5, b'ab', [(L, 2)]))


CASES['binary_47'] = _binary_case(47)          # the copies part in the second text round (depth 48) ...
CASES['binary_48'] = _binary_case(48)          # ... or need a third
EDGES.append(('binary_47', 'binary_48'))


# -- PSS_TEXT_ROUNDS: ties that need six text rounds

def _six_rounds_text(n=N16 + 9):
    return plant(400, n, E.FILL39, [(K8 + 5 * 10 + 3, 2)] + _decoys(K8 + 5 * 10 + 3, K8, 10, 6))


def _cap_case(cap):
    switches = {'PSS_MODE': 'text'}
    if cap is not None:
        switches['PSS_TEXT_ROUNDS'] = str(cap)

    def make():
        t = _six_rounds_text()
        free = _w(t, K8, {'PSS_MODE': 'text', 'PSS_TEXT_ROUNDS': '9'})
        assert [r.kind for r in free.rounds_list] == ['text'] * 6, str(free)
        w = _w(t, K8, switches)
        c = TEXT_ROUNDS_DEFAULT if cap is None else cap
        assert [r.kind for r in w.rounds_list[:c + 1]] == ['text'] * c + ['rank'], str(w)
        assert w.rounds_list[c].h == K8 + c * 10, str(w)       # the rank round starts at the depth the text rounds reached
        return t
    return Case(make, K8, switches, lambda: _six_rounds_text(SMALL + 9))


for _cap in (0, 1, 2, None):
    CASES['text_rounds_%s' % ('default' if _cap is None else _cap)] = _cap_case(_cap)
EDGES += [('text_rounds_0', 'text_rounds_1'), ('text_rounds_1', 'text_rounds_2'), ('text_rounds_2', 'text_rounds_default')]


# -- text_progress: the second text round starts with exactly 6/10 of the first one's list, or with one pair less before

def _progress_case(pairs):
    """One word of 8 + 10 + 29 symbols twice: 80 members in the first round, 60 in the second.  `pairs` words of 8 symbols
    twice: 2 members each in the first round only.  60 * 10 <= (80 + 2 pairs) * 6 iff pairs >= 10."""
    switches = {'PSS_MODE': 'text'}

    def text(n):
        return plant(500, n, E.FILL39, [(K8 + 10 + 29, 2)] + [(K8, 2)] * pairs)

    def make():
        t = text(N16 + 3)
        w = _w(t, K8, switches)
        r0, r1 = w.rounds_list[:2]
        assert (r0.kind, r0.m, r1.m) == ('text', 80 + 2 * pairs, 60), str(w)
        assert r1.kind == ('text' if pairs >= 10 else 'rank') and (r1.m * 10 <= r0.m * 6) == (pairs >= 10), str(w)
        return t
    return Case(make, K8, switches, lambda: text(SMALL + 3))


CASES['progress_at'] = _progress_case(10)
CASES['progress_above'] = _progress_case(9)
EDGES.append(('progress_at', 'progress_above'))


# -- large groups: a word written K_BIG times is a group beyond the middle tier at every place of the word the depth leaves tied

K_BIG = 4098         # (> MID_CAP, and a multiple of 3)
N18 = (1 << 18) - 7


def _tuned(seed, n, families, switches, at_round, target, filler_len):
    """The families, and words of filler_len symbols written twice or three times until the round's list holds
    target(nbig) members exactly."""
    extra = 0
    for _ in range(8):
        c = extra % 2
        fam = list(families) + [(filler_len, 2)] * ((extra - 3 * c) // 2) + [(filler_len, 3)] * c
        t = plant(seed, n, E.FILL39, fam)
        r = _w(t, K8, switches).rounds_list[at_round]
        want = target(r.nbig)
        if r.m == want:
            return t
        extra += want - r.m
        assert extra >= 0 and extra != 1, (extra, r)
    raise AssertionError('no text with %d members' % want)


def _give_up_first(over):
    """First text round: the large groups hold exactly 3/4 of the list (the round runs), or 2 members more than 3/4 of
    it (it gives up: nothing of it counts, rank rounds from the same depth)."""
    switches = {'PSS_MODE': 'text'}

    def make():
        t = _tuned(600, N18, [(K8 + 12, K_BIG)], switches, 0, lambda nbig: nbig * 4 // 3 - (2 if over else 0), K8)
        w = _w(t, K8, switches)
        r = w.rounds_list[0]
        assert r.kind == 'text' and r.nbig == 13 * K_BIG and r.gave_up == over and (r.nbig * 4 > r.m * 3) == over, str(w)
        assert w.rounds_list[1].kind == ('rank' if over else 'text') and w.rounds_list[1].h == (K8 if over else K8 + 10), str(w)
        return t
    return Case(make, K8, switches)


def _give_up_later(over):
    """Second text round: the large groups hold exactly 1/2 of its list, or 2 members more than that."""
    switches = {'PSS_MODE': 'text'}

    def make():
        # at depth 18 the word of 22 is tied at 5 places (large groups) and two places before and behind it (small ones);
        # the word of 16, written 2000 times, is in the first round's list only, and keeps that round from giving up
        t = _tuned(700, N18, [(K8 + 10 + 4, K_BIG), (K8 + 8, 2000)], switches, 1, lambda nbig: nbig * 2 - (2 if over else 0), K8 + 10)
        w = _w(t, K8, switches)
        r0, r = w.rounds_list[:2]
        assert r0.kind == 'text' and not r0.gave_up and r.kind == 'text' and r.h == K8 + 10, str(w)
        assert r.nbig == 5 * K_BIG and r.gave_up == over and (r.nbig * 2 > r.m) == over, str(w)
        assert not over or (w.rounds_list[2].kind, w.rounds_list[2].h) == ('rank', K8 + 10), str(w)
        return t
    return Case(make, K8, switches)


CASES['give_up_first_at'], CASES['give_up_first_over'] = _give_up_first(False), _give_up_first(True)
CASES['give_up_later_at'], CASES['give_up_later_over'] = _give_up_later(False), _give_up_later(True)
EDGES += [('give_up_first_at', 'give_up_first_over'), ('give_up_later_at', 'give_up_later_over')]


def _global_edge(over):
    """PSS_MODE=dense: the large groups of the first rank round hold exactly half of the list (the rounds stay local), or
    2 members more (global rounds while the list is longer than half of this one).  A second word, written 2000 times,
    keeps more than half of the list tied at depth 16: the second round is local on one side and global on the other."""
    switches = {'PSS_MODE': 'dense'}

    def make():
        t = _tuned(800, N18, [(K8 + 12, K_BIG), (K8 + 13, 2000)], switches, 0, lambda nbig: nbig * 2 - (2 if over else 0), K8)
        w = _w(t, K8, switches)
        r, r1 = w.rounds_list[:2]
        assert r.kind == 'rank' and r.nbig == 13 * K_BIG and (r.nbig * 2 > r.m) == over, str(w)
        assert r1.m > r.m // 2 and r1.kind == ('global' if over else 'rank') and (over or r1.nbig == 5 * K_BIG), str(w)
        return t
    return Case(make, K8, switches)


def _global_then_local():
    """PSS_MODE=dense, a word of 40 symbols K_BIG times: the list of the first round is nearly all large groups, the second
    (depth 16) still holds more than half of it -- a global round -- and the third (depth 32) does not: local again."""
    switches = {'PSS_MODE': 'dense'}

    def make():
        t = plant(900, N18, E.FILL39, [(40, K_BIG)])
        w = _w(t, K8, switches)
        assert [r.kind for r in w.rounds_list[:3]] == ['rank', 'global', 'rank'], str(w)
        r0, r1, r2 = w.rounds_list[:3]
        assert r1.m > r0.m // 2 >= r2.m and r2.nbig > 0, str(w)
        return t
    return Case(make, K8, switches)


def _dominating():
    """Random text over two symbols, one symbol per key: every suffix but the last is in one of two groups."""
    def make():
        rng = np.random.default_rng(1000)
        t = np.append(np.frombuffer(b'ab', dtype=np.uint8)[rng.integers(0, 2, N16 + 10)], np.uint8(E.NL))
        w = _w(t, 1, {})
        assert w.rounds_list[0] == Round('text', 1, t.size - 1, t.size - 1, True) and w.rounds_list[1].kind == 'rank', str(w)
        assert [r.kind for r in w.rounds_list[2:]] == ['global'] * (len(w.rounds_list) - 2), str(w)      # (the list never halves)
        return t
    return Case(make, 1, {})


CASES['global_at'], CASES['global_over'] = _global_edge(False), _global_edge(True)
CASES['global_then_local'] = _global_then_local()
CASES['dominating'] = _dominating()
EDGES.append(('global_at', 'global_over'))


# -- the tiers: E.tier_case under the variants of tests/test_sa_edges_gpu.py the model covers (all but anchor1)

TIER_SHAPES = ('plain', 'second', 'crowded')
TIER_KEY_CHARS = 6
_TIER_WALKS = {}


def tier_walk(k, shape, switches, text=None, params=None):
    """The walk of E.tier_case(k, shape) under the switches (made once per initial key and set of switches the walk
    depends on; by default the key of PSS_KEY_CHARS=6)."""
    t = E.tier_case(k, shape) if text is None else text
    params = params_of(t, TIER_KEY_CHARS) if params is None else params
    key = (k, shape, walk_key(switches), tuple(sorted(params.items())))
    if key not in _TIER_WALKS:
        _TIER_WALKS[key] = walk(t, switches=switches, **params)
    return _TIER_WALKS[key]


# ---- independent references (tests/test_rounds_model.py) -----------------------------------------------------------------

def brute_ranks(text, d):
    """1 + the number of suffixes whose zero-padded prefix of d symbols is smaller: by sorting the prefixes themselves."""
    codes, _ = recode(text)
    raw = codes.astype(np.uint8).tobytes() + bytes(d)
    n = codes.size
    pre = [raw[i:i + d] for i in range(n)]
    order = sorted(range(n), key=pre.__getitem__)
    rank = np.empty(n, np.int64)
    head = 0
    for slot, i in enumerate(order):
        if slot and pre[i] != pre[order[slot - 1]]:
            head = slot
        rank[i] = head + 1
    return rank


def kasai(text, sa):
    """LCP of neighbours in the suffix array (Kasai et al.), written directly."""
    t = np.ascontiguousarray(text).tolist()
    sa = np.asarray(sa).tolist()
    n = len(t)
    isa = [0] * n
    for slot, i in enumerate(sa):
        isa[i] = slot
    lcp = [0] * n
    h = 0
    for i in range(n):
        if isa[i] == 0:
            h = 0
            continue
        j = sa[isa[i] - 1]
        while i + h < n and j + h < n and t[i + h] == t[j + h]:
            h += 1
        lcp[isa[i]] = h
        if h:
            h -= 1
    return lcp
