"""The anchor round on its edges (csrc/anchor_impl.h, AnchorRound in csrc/anchor_driver_impl.h): the three code paths of
anc_select_kernel by window (the plain loop up to 8, anc_window_mins<9> + <8> up to 16, anc_window_mins<17> above) and their
seams, the host's clamp to 64, tile borders and the end of the text (the partial uint4 of d and of the key fill, hashes
that read the padding), the refusal below 64 bytes, the limit of n / div anchors from both sides, and a second level of
anchors on top of the first.

Suffix-array equality cannot see a wrong selection -- any content-defined choice of anchors gives the exact result -- so
every build is also held to the numpy model of tests/anchor_texts.py: the window is the host rule's for the depth the build
reports, the number of anchors is the model's for that window, to the element, and the round runs exactly when the model
says so.  tests/test_anchor_texts.py checks the model and the texts without a GPU.  Every suffix array is compared with
the oracle's for equality: it is unique, there is no tolerance."""
import numpy as np
import pytest

from tests import anchor_texts as A
from tests.util import sa_device

pytestmark = pytest.mark.gpu

_CACHE = {}
COMMON = dict(PSS_ANCHOR=1, PSS_MODE='text', PSS_RLE=0, PSS_PERIOD=0, PSS_NO_PROBE=1)
KNOBS = ('PSS_ANCHOR_OMEGA', 'PSS_ANCHOR_CAP_DIV', 'PSS_ANCHOR_SIDE', 'PSS_KEY_CHARS', 'PSS_TEXT_ROUNDS', 'PSS_PERIODIC')
# 63 .. 65 bytes: no tie outlives the default key and a text round of 16 symbols, and a round that resolves 40 % earns another;
# a key of 2 symbols and ONE text round leave the copies of 24 bytes tied when the build asks for the anchors
TINY = dict(PSS_KEY_CHARS=2, PSS_TEXT_ROUNDS=1)
FORCED = (None, 2, 3, 8, 9, 16, 17, 33)


def _case(oracle, key, make):
    """(text, the oracle's suffix array, the codes of the model): made once per session, never written to."""
    if key not in _CACHE:
        t = np.array(make(), dtype=np.uint8)          # (a copy: the generators keep theirs)
        want = oracle.sa(t)
        want.setflags(write=False)
        _CACHE[key] = (t, want, A.codes_of(t))
    return _CACHE[key]


def _tiled(oracle, n, alpha):
    return _case(oracle, ('tiled', n, alpha), lambda: A.tiled(n, alpha))


def _count(case, omega, w):
    key = ('count', id(case[0]), omega, w)
    if key not in _CACHE:
        _CACHE[key] = A.anchor_count(case[2], omega, w)
    return _CACHE[key]


def _build(monkeypatch, case, forced=None, note=None, flags=8, side=False, **env):
    """One forced cold build: the oracle's bytes, nothing left tied, and the model's window, count and decision."""
    t, want = case[:2]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(COMMON, **env).items():
        monkeypatch.setenv(k, str(v))
    if forced:
        monkeypatch.setenv('PSS_ANCHOR_OMEGA', str(forced))
    st = {}
    sa = sa_device(np.asarray(t), st, flags=flags)
    note = (note, t.size, forced, env)
    depth = A.depth_of(st)
    got = {k: int(st[k]) for k in ('anchor', 'anchor_omega', 'anchor_w', 'anchor_count', 'anchor_depth', 'anchor_levels', 'anchor_side')}
    print(note, 'depth', depth, 'text rounds', st['text_rounds'], got)
    assert np.array_equal(sa, want), note
    assert st['anchor_left'] == 0 and st['rle'] == 0 and st['period_path'] == 0, note
    if side and st['anchor_side'] == 1:
        # made beside the text round, for the depth that round was expected to reach: never a wider window than the depth allows
        assert 2 <= got['anchor_omega'] <= A.window_of(got['anchor_depth'], forced).omega and got['anchor_w'] in (4, 8), note
        assert got['anchor'] == 1 and got['anchor_count'] == _count(case, got['anchor_omega'], got['anchor_w']), note
        return st
    win = A.window_of(depth, forced)
    if win.omega < 2 or t.size < A.MIN_N:
        assert got['anchor'] == 0 and got['anchor_count'] == 0, note      # refused before anything is selected
        return st
    assert (got['anchor_omega'], got['anchor_w']) == win, (note, depth)
    model = _count(case, win.omega, win.w)
    assert got['anchor_count'] == model, (note, depth, win, model)
    runs = A.runs(t.size, win.omega, model, env.get('PSS_ANCHOR_CAP_DIV', 5))
    assert got['anchor'] == (1 if runs else 0), (note, win, model)
    if runs:
        assert got['anchor_depth'] == depth and got['anchor_levels'] >= 1, note
    return st


def _env_of(n):
    return TINY if n <= 66 else {}


# ---- windows by code path --------------------------------------------------------------------------------------------

def test_every_window_path_over_tile_and_text_edges(oracle, monkeypatch):
    """tiled() at every length (64, 65, around one tile of 4096 window starts and its 16-position groups, two tiles, three
    and five bytes) and alphabet (2, 4, 39 symbols, all 256 byte values), with the window forced to 2, 3, 8 | 9, 16 | 17, 33
    and left to the depth.  Where the depth allows less than the forced window the build is held to the window it ran with.
    The ladder (depth >= 79) supplies the forced window of 33 where the tiled texts stop short of it.  At the end: the windows
    that ran cover the plain loop, both halves of the middle path and the wide one, and both seams."""
    ran = {}
    cases = [(_tiled(oracle, n, alpha), (n, alpha), _env_of(n)) for alpha in sorted(A.ALPHABETS) for n in A.TILED_NS]
    for forced in FORCED:
        for case, note, env in cases:
            st = _build(monkeypatch, case, forced, note, **env)
            assert st['anchor_count'] > 0, (note, forced)          # the build asked for the anchors: the text reached the round
            ran.setdefault(int(st['anchor_omega']), set()).add(note[1])
    st = _build(monkeypatch, _case(oracle, ('ladder',), A.ladder), 33, 'ladder')
    assert st['anchor'] == 1
    ran.setdefault(int(st['anchor_omega']), set()).add('ladder')
    print('windows that ran:', {k: sorted(map(str, v)) for k, v in sorted(ran.items())})
    assert {2, 3, 8, 9, 16, 17, 33} <= set(ran), sorted(ran)
    assert set(ran[2]) >= set(A.ALPHABETS)                         # every alphabet took the plain loop, 256 raw bytes included


def test_raw_bytes_take_the_round(oracle, monkeypatch):
    """All 256 byte values: 9-bit codes, a key of 4 symbols and a text round of 7 -- the depth allows a window of 8 at most,
    which chooses more than n / 5 anchors, so the builds above count them and decline.  With the limit at n / 4 they run:
    the anchors' names and the key fill over raw bytes, byte 0 among them, give the oracle's bytes."""
    for n in A.TILED_NS:
        if n >= 4095:
            st = _build(monkeypatch, _tiled(oracle, n, 256), None, (n, 256), PSS_ANCHOR_CAP_DIV=4)
            assert st['sigma'] == 256 and st['anchor'] == 1, n


def test_the_clamp_to_64(oracle, monkeypatch):
    """The ladder drains slowly enough for four or five text rounds of 16 symbols: the depth allows more than 64, unforced
    and with PSS_ANCHOR_OMEGA=65, and the window is 64 over hashes of 8 bytes."""
    case = _case(oracle, ('ladder',), A.ladder)
    A.check_ladder(case[0], case[1])
    for forced in (None, 65):
        st = _build(monkeypatch, case, forced, 'ladder')
        assert st['anchor_depth'] >= 71 and st['anchor'] == 1
        assert st['anchor_omega'] == 64 and st['anchor_w'] == 8


@pytest.mark.parametrize('alpha', sorted(A.ALPHABETS))
def test_63_64_65_bytes(oracle, monkeypatch, alpha):
    """Below 64 bytes the round is refused before anything is selected (the rank rounds finish the build); 64 and 65 take it.
    So short a text has one anchor in about five positions whatever the window -- its last window alone chooses several --
    so the limit is set to n / 3, the widest the knob allows; the model decides, as everywhere."""
    env = dict(TINY, PSS_ANCHOR_CAP_DIV=3)
    st = _build(monkeypatch, _tiled(oracle, A.REFUSED_N, alpha), None, alpha, **env)
    assert st['anchor'] == 0 and st['anchor_count'] == 0 and st['text_rounds'] == 1 and st['rounds'] > 1
    for n in (64, 65):
        st = _build(monkeypatch, _tiled(oracle, n, alpha), None, alpha, **env)
        assert st['anchor'] == 1 and 0 < st['anchor_count'] <= n // 3, (n, alpha)


def test_stale_padding_behind_a_shorter_text(oracle, monkeypatch):
    """After a text of 70 001 bytes the same context builds texts with n % 16 = 1, 9 and 15 under hashes of 8 bytes, which read
    seven bytes past the last position: they must hash zeros there, as the model does, not what the longer text left."""
    _build(monkeypatch, _tiled(oracle, A.LONG_N, 39), None, 'long')
    for n in A.STALE_NS:
        assert n % 16 in (1, 9, 15)
        st = _build(monkeypatch, _tiled(oracle, n, 4), None, 'short')
        assert st['anchor'] == 1 and st['anchor_w'] == 8
        _build(monkeypatch, _tiled(oracle, A.LONG_N, 39), 9, 'long')


@pytest.mark.parametrize('alpha', sorted(A.ALPHABETS))
def test_beside_the_text_round(oracle, monkeypatch, alpha):
    """PSS_ANCHOR_SIDE=1: the anchors are selected and sorted beside the text round, for the depth it is expected to reach.
    When the side line's keys are used the count is the model's for the window it reports; a second build of the same text
    (the plan the first one left) must agree."""
    case = _tiled(oracle, 8193, alpha)
    seen = []
    for forced in (None, 12):
        for flags in (8, 0):
            st = _build(monkeypatch, case, forced, alpha, flags=flags, side=True, PSS_ANCHOR_SIDE=1)
            assert st['anchor_side'] in (1, 2)                     # the side line started: used, or thrown away and selected again
            seen.append((forced, int(st['anchor_side']), int(st['anchor_omega']), int(st['anchor_w']), int(st['anchor_count'])))
    print(alpha, seen)
    assert seen[0][2:] == seen[1][2:] and seen[2][2:] == seen[3][2:]


@pytest.mark.parametrize('div', A.CAP_DIVS)
def test_on_the_cap(oracle, monkeypatch, div):
    """Two prefixes of one text: the one whose windows choose exactly n // div anchors runs the round, the one with one
    anchor more declines it after the count, and the rank rounds give the same bytes.  PSS_ANCHOR_CAP_DIV clamps to 3 .. 5,
    and 5 is what a build without the knob uses."""
    omega, on, over = A.on_the_cap(div, A.CAP_W)
    knobs = [dict(PSS_ANCHOR_CAP_DIV=div)]
    if div == 5:
        knobs += [{}, dict(PSS_ANCHOR_CAP_DIV=9)]
    if div == 3:
        knobs += [dict(PSS_ANCHOR_CAP_DIV=1)]
    for env in knobs:
        a = _build(monkeypatch, _case(oracle, ('cap', div, 0), lambda: on), omega, ('on', div), **env)
        assert a['anchor_w'] == A.CAP_W and a['anchor_omega'] == omega
        assert a['anchor'] == 1 and a['anchor_count'] == on.size // div
        b = _build(monkeypatch, _case(oracle, ('cap', div, 1), lambda: over), omega, ('over', div), **env)
        assert b['anchor_w'] == A.CAP_W and b['anchor_omega'] == omega
        assert b['anchor'] == 0 and b['anchor_count'] == over.size // div + 1


@pytest.mark.parametrize('periodic', [None, 0])
@pytest.mark.parametrize('alpha', A.DEEP_ALPHAS)
def test_levels(oracle, monkeypatch, alpha, periodic):
    """Copies of n / 8 bytes: the names of the anchors repeat as the text does, the rank rounds over them reach depth 32 with
    most of them tied, and minimizers of the NAMES (anc_select_kernel<true>, the `syms` branch of AnchorRound) go on top:
    anchor_levels counts them.  Observed on an MI355X at n = 2^18, with PSS_PERIODIC at its default and at 0 alike: 4 symbols
    (depth 32, window 25, 8-byte hashes, 19 970 anchors) three levels, 39 symbols (depth 16, window 13, 4-byte hashes, 37 552
    anchors) three levels -- so three are asked of all four cases."""
    env = {} if periodic is None else dict(PSS_PERIODIC=periodic)
    st = _build(monkeypatch, _case(oracle, ('deep', alpha), lambda: A.deep(A.DEEP_N, alpha)), None, ('deep', alpha), **env)
    assert st['anchor'] == 1
    assert st['anchor_levels'] >= 2, st['anchor_levels']
    assert st['anchor_levels'] >= 3, st['anchor_levels']
