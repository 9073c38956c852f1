"""msd_finish_kernel (msd_sort.hip): tied groups of up to FIN_MAX suffixes that one more 64-bit text key separates are
written to their final slots between the local sort and the gather; every other group reaches the rounds whole.  The
texts and the numpy model of the rule are in tests/msd_finish_texts.py: a CPU-side assert checks that every planted
group is what its case is about, `msd_finished` must be exactly the model's count, and every suffix array is compared
with the oracle's for equality."""
import numpy as np
import pytest

from tests import msd_finish_texts as F
from tests.util import sa_device

pytestmark = pytest.mark.gpu

FIN_MAX = F.FIN_MAX
_CACHE = {}

ROUTES = {'default': {}, 'msd_order': {'PSS_MSD_LSD': '0'}, 'slow_local': {'PSS_MSD_SLOW_LOCAL': '1'},
          'no_fuse': {'PSS_MSD_NO_FUSE': '1'}, 'no_finish': {'PSS_MSD_NO_FINISH': '1'}}
FORMATS = {'cap42': dict(cap=42), 'cap40': dict(cap=40), 'default': dict(), 'partial43': dict(cap=43, partial=True)}


def _env(monkeypatch, fmt=None, **kv):
    monkeypatch.setenv('PSS_MSD', '1')
    monkeypatch.setenv('PSS_PERIOD', '0')
    if fmt and 'cap' in fmt:
        monkeypatch.setenv('PSS_MSD_KEY_CAP', str(fmt['cap']))
    if fmt and fmt.get('partial'):
        monkeypatch.setenv('PSS_MSD_PARTIAL_SYMBOL', '1')
    for k, v in kv.items():
        monkeypatch.setenv(k, str(v))


def _case(oracle, key, make):
    """(text, facts about it, the oracle's suffix array): made once per session, never written to."""
    if key not in _CACHE:
        t, facts = make()
        t = np.ascontiguousarray(t)
        want = oracle.sa(t)
        want.setflags(write=False)
        t.setflags(write=False)
        _CACHE[key] = (t, facts, want)
    return _CACHE[key]


def _model(key, t, fmt):
    k = ('model', key, tuple(sorted(fmt.items())))
    if k not in _CACHE:
        f = F.Format(t.size, int(np.unique(t).size), **fmt)
        _CACHE[k] = (f, F.Model(t, f))
    return _CACHE[k]


def _build(t, want, f, note=None):
    st = {}
    sa = sa_device(np.asarray(t), st)
    assert np.array_equal(sa, want), note
    assert st['msd'] == 1 and st['rle'] == 0 and st['period_path'] == 0, note
    assert (st['code_bits'], st['key_chars'], st['key_bits']) == (f.b, f.kc, f.kb), note      # the model's format is the sort's
    return st


def _check_stats(st, m, finishing=True, note=None):
    print(note, 'finished', st['msd_finished'], 'model', m.n_finished, 'left', m.n_left, 'sum_active', st['sum_active'],
          'rounds', st['rounds'])
    if finishing:
        assert st['msd_finished'] == m.n_finished, note
        assert st['sum_active'] >= m.n_left and (st['sum_active'] > 0) == (m.n_left > 0), note
    else:
        assert st['msd_finished'] == 0, note
        assert st['sum_active'] >= m.n_left + m.n_finished, note


# ---- the texts -------------------------------------------------------------------------------------------------------

def _group(t, rng, taken, alpha, shared, g):
    """g copies of one word of `shared` symbols, each followed by a symbol of its own: a group of g that first differs at
    symbol shared + 1."""
    w = F.word(rng, alpha, shared)
    return F.plant(t, rng, [w + x for x in F.distinct_symbols(rng, alpha, g)], taken)


def sizes_text():
    """Case 1: groups of exactly 2, 3, FIN_MAX and FIN_MAX + 1 that share h0 symbols and differ at symbol h0 + 1."""
    rng = np.random.default_rng(101)
    n, alpha = 131101, 39
    f = F.Format(n, alpha + 1)
    t = F.background(rng, n, alpha)
    taken = []
    groups = {g: _group(t, rng, taken, alpha, f.h0, g) for g in (2, 3, FIN_MAX, FIN_MAX + 1)}
    m = F.Model(t, F.Format(n, int(np.unique(t).size)))
    for g, at in groups.items():
        for p in at:
            assert m.size[p] == g and m.finished[p] == (g <= FIN_MAX), (g, p)
            assert p == at[0] or m.first_difference(at[0], p) == f.h0, (g, p)
    return t, groups


def depth_text():
    """Case 2: pairs that first differ at symbol h0 + 1, at the last symbol of the extra key and one symbol past it; three
    suffixes of which two share the extra key."""
    rng = np.random.default_rng(202)
    n, alpha = 98317, 39
    f = F.Format(n, alpha + 1)
    t = F.background(rng, n, alpha)
    taken = []
    facts = {}
    for name, shared in (('first', f.h0), ('last', f.h0 + f.ks - 1), ('past', f.h0 + f.ks)):
        facts[name] = _group(t, rng, taken, alpha, shared, 2)
    w, (e1, e2) = F.word(rng, alpha, f.h0), F.distinct_symbols(rng, alpha, 2)
    rest = F.word(rng, alpha, f.ks - 1)
    y1, y2 = F.distinct_symbols(rng, alpha, 2)
    facts['two_of_three'] = F.plant(t, rng, [w + e1 + rest + y1, w + e1 + rest + y2, w + e2], taken)
    m = F.Model(t, F.Format(n, int(np.unique(t).size)))
    for name, shared in (('first', f.h0), ('last', f.h0 + f.ks - 1), ('past', f.h0 + f.ks)):
        a, b = facts[name]
        assert m.size[a] == m.size[b] == 2 and m.first_difference(a, b) == shared, name
        assert m.finished[a] == m.finished[b] == (name != 'past'), name
    a, b, c = facts['two_of_three']
    assert m.size[a] == m.size[b] == m.size[c] == 3 and not m.finished[a] and not m.finished[c]
    assert m.first_difference(a, b) == f.h0 + f.ks and m.first_difference(a, c) == f.h0
    return t, facts


def end_text():
    """Case 3: the text ends with a word of h0 symbols and three more bytes, and holds a copy of all that followed by more
    text -- a pair at every shift: one suffix ends inside the extra key (shifts 0 .. 2) or exactly at h0 (shift 3).  Two
    suffixes that start with the largest byte tie as well: the last two slots of the suffix array, the last tile."""
    rng = np.random.default_rng(303)
    n, alpha = 70001, 39
    f = F.Format(n, alpha + 2)                        # (+ '\n' and the lead byte)
    t = F.background(rng, n, alpha)
    x = F.word(rng, alpha, f.h0 + 2) + bytes([F.NL])
    t[n - len(x):] = np.frombuffer(x, np.uint8)
    taken = [(n - len(x), n)]
    (p,) = F.plant(t, rng, [x], taken)
    lead = bytes([F.LEAD]) + F.word(rng, alpha, f.h0 - 1)
    tail = F.plant(t, rng, [lead + s for s in F.distinct_symbols(rng, alpha, 2)], taken)
    m = F.Model(t, F.Format(n, int(np.unique(t).size)))
    for s in range(4):
        a, b = n - len(x) + s, p + s
        assert m.size[a] == m.size[b] == 2 and m.finished[a], s
        assert n - a == f.h0 + 3 - s and m.first_difference(a, b) == n - a      # (one of them ends: code 0 against a symbol)
    assert sorted(m.slot[tail]) == [n - 2, n - 1] and m.size[tail[0]] == 2 and m.finished[tail[0]]
    return t, {'end': (n - len(x), p), 'tail': tail}


_ALPHA_N = {4: 70001, 39: 131075, 200: 300007}


def format_text(alpha):
    """Case 4: a random text over alpha byte values with a pair, a triple and a group of FIN_MAX + 1 that share one symbol
    more than the widest key format compares whole (tied under every format of FORMATS, apart within the extra key), and
    a pair that goes on alike beyond the extra key of every format."""
    rng = np.random.default_rng(400 + alpha)
    n = _ALPHA_N[alpha]
    wide = F.Format(n, alpha + 1)
    shared = wide.h0 + 1
    t = F.background(rng, n, alpha)
    taken = []
    if alpha >= FIN_MAX + 1:
        facts = {g: _group(t, rng, taken, alpha, shared, g) for g in (2, 3, FIN_MAX + 1)}
    else:           # (four symbols: a group cannot have five members that differ at one symbol)
        facts = {g: _group(t, rng, taken, alpha, shared, g) for g in (2, 3)}
    facts['deep'] = _group(t, rng, taken, alpha, wide.h0 + wide.ks + 1, 2)
    return t, facts


def _format_facts(t, facts, f, m):
    for g, at in facts.items():
        for p in at:
            if g == 'deep':
                assert m.size[p] == 2 and not m.finished[p], (g, p)
            else:
                assert m.size[p] == g and m.finished[p] == (g <= FIN_MAX), (g, p)


def chained_text():
    """Pairs that share 24 symbols: the pair itself is left to the rounds (its extra key covers symbols 9 .. 18), the same
    two suffixes 8 and 16 symbols on are finished pairs -- and they are what the rank rounds look up at h = 8 and h = 16."""
    rng = np.random.default_rng(707)
    n, alpha = 90007, 39
    f = F.Format(n, alpha + 1)
    assert (f.h0, f.ks) == (8, 10)
    t = F.background(rng, n, alpha)
    taken = []
    pairs = [_group(t, rng, taken, alpha, 24, 2) for _ in range(12)]
    m = F.Model(t, F.Format(n, int(np.unique(t).size)))
    for a, b in pairs:
        assert m.size[a] == 2 and not m.finished[a] and m.first_difference(a, b) == 24
        for h in (8, 16):
            assert m.size[a + h] == 2 and m.finished[a + h] and m.finished[b + h]
    return t, pairs


def nothing_left_text():
    """Case 6: a random 39-symbol text of 2^18 + 3 bytes all of whose ties (at 42 key bits) fall to the finisher."""
    rng = np.random.default_rng(NOTHING_LEFT_SEED)
    t = F.background(rng, (1 << 18) + 3, 39)
    return t, {}


NOTHING_LEFT_SEED = 600


# ---- the tests -------------------------------------------------------------------------------------------------------

def test_group_sizes(oracle, monkeypatch):
    """Groups of 2, 3 and FIN_MAX members are finished, the group of FIN_MAX + 1 comes through the rounds."""
    _env(monkeypatch)
    t, groups, want = _case(oracle, 'sizes', sizes_text)
    f, m = _model('sizes', t, {})
    st = _build(t, want, f)
    _check_stats(st, m, note='sizes')
    assert st['msd_finished'] >= 2 + 3 + FIN_MAX and st['sum_active'] >= FIN_MAX + 1


def test_where_the_members_differ(oracle, monkeypatch):
    """A difference at the first and at the last symbol of the extra key finishes the pair; one symbol past it, or two equal
    extra keys among three members, leaves the whole group to the rounds."""
    _env(monkeypatch)
    t, facts, want = _case(oracle, 'depth', depth_text)
    f, m = _model('depth', t, {})
    st = _build(t, want, f)
    _check_stats(st, m, note='depth')
    assert st['sum_active'] >= 2 + 3


def test_end_of_text(oracle, monkeypatch):
    """One member ends inside the extra key, or exactly where it starts (its key is 0: nothing of the text is read); a
    pair in the last slots of the last tile."""
    _env(monkeypatch)
    t, facts, want = _case(oracle, 'end', end_text)
    f, m = _model('end', t, {})
    st = _build(t, want, f)
    _check_stats(st, m, note='end')
    assert st['msd_finished'] >= 2 * 4 + 2


@pytest.mark.parametrize('fmt', list(FORMATS))
@pytest.mark.parametrize('alpha', [4, 39, 200])
def test_code_widths_and_key_formats(oracle, monkeypatch, alpha, fmt):
    """3-, 6- and 8-bit codes (extra keys of 16, 10 and 8 symbols) under key caps of 42, 40 and 48 bits and with a partly
    compared last symbol (PSS_MSD_PARTIAL_SYMBOL: the extra key starts AT that symbol, h0 = key_chars - 1)."""
    _env(monkeypatch, FORMATS[fmt])
    t, facts, want = _case(oracle, ('format', alpha), lambda: format_text(alpha))
    f, m = _model(('format', alpha), t, FORMATS[fmt])
    _format_facts(t, facts, f, m)
    if fmt == 'partial43':
        assert f.drop != 0 and f.h0 == f.kc - 1
    st = _build(t, want, f, (alpha, fmt))
    _check_stats(st, m, note=(alpha, fmt))
    assert st['msd_finished'] >= 2 + 3 and st['sum_active'] >= 2


@pytest.mark.parametrize('route', [r for r in ROUTES if r != 'default'])
@pytest.mark.parametrize('text', ['sizes', 'depth'])
def test_every_route(oracle, monkeypatch, text, route):
    """The texts of the first two cases with the digits in MSD order, the general local-sort kernel, ties flagged in the
    suffix array (no records: nothing to finish) and the finisher switched off: the same bytes, and nothing finished
    under the last two."""
    _env(monkeypatch, **ROUTES[route])
    t, facts, want = _case(oracle, text, {'sizes': sizes_text, 'depth': depth_text}[text])
    f, m = _model(text, t, {})
    st = _build(t, want, f, (text, route))
    _check_stats(st, m, finishing=route not in ('no_fuse', 'no_finish'), note=(text, route))


@pytest.mark.parametrize('mode', ['chosen', 'sparse', 'dense', 'text'])
def test_rounds_look_up_finished_suffixes(oracle, monkeypatch, mode):
    """The rounds rank a group that was left whole by the suffixes h symbols on -- which the finisher has placed: they
    are not in the active list, yet share their sort key with the other members of their finished group.  The sparse
    mode (chosen by itself when few suffixes are left) finds such a suffix by its key and must end on its own slot."""
    _env(monkeypatch)
    if mode != 'chosen':
        monkeypatch.setenv('PSS_MODE', mode)
    t, pairs, want = _case(oracle, 'chained', chained_text)
    f, m = _model('chained', t, {})
    st = _build(t, want, f, mode)
    _check_stats(st, m, note=('chained', mode))
    assert st['sum_active'] >= 2 * len(pairs)


def test_nothing_left(oracle, monkeypatch):
    """Every tie of the text falls to the finisher: the rounds have nothing to do -- no round, no active suffix, which is
    what a build of a text without any tie reports (the loop of Rounds::run leaves before it counts a round)."""
    _env(monkeypatch, FORMATS['cap42'])
    t, _, want = _case(oracle, 'nothing', nothing_left_text)
    f, m = _model('nothing', t, FORMATS['cap42'])
    assert m.n_finished > 0 and m.n_left == 0          # (the seed was chosen for this)
    st = _build(t, want, f)
    _check_stats(st, m, note='nothing left')
    assert st['sum_active'] == 0 and st['rounds'] == 0
    # a text without ties, for comparison
    rng = np.random.default_rng(601)
    u = F.background(rng, 70001, 200)
    mu = F.Model(u, F.Format(u.size, int(np.unique(u).size)))
    assert mu.n_finished == 0 and mu.n_left == 0
    su = {}
    assert np.array_equal(sa_device(u, su), oracle.sa(u))
    assert (su['sum_active'], su['rounds'], su['msd_finished']) == (0, 0, 0)
