"""The rounds of the builder (sa_refine_impl.h driving the kernels of sa_rounds_impl.h and sa_rerank_impl.h) against the
CPU model of tests/rounds_model.py: for every text that puts one decision of the driver on its edge -- the mode, the
depth a round leaves, the cap and the progress of the text rounds, a text round giving up, the list going global and
coming back, the group-size tiers -- the suffix array equals the oracle's, and the counts the build reports (rounds,
text_rounds, sum_active, big_elems, mode) equal the model's.  They are counts: there is no tolerance.  A suffix array
is unique, so rounds that waste work still end on the right bytes; these totals are what says which decision moved.
tests/test_rounds_model.py holds the model itself to a brute force, on the CPU."""
import numpy as np
import pytest

from pysubstringsearch_amd import _ffi
from tests import rle_texts as R
from tests import rounds_model as M
from tests import sa_edge_texts as E
from tests.util import sa_device

pytestmark = pytest.mark.gpu

_ORACLE = {}
OFF = ('msd', 'ss', 'rle', 'anchor', 'periodic_rounds')


def _want(oracle, key, t):
    """The oracle's suffix array of a case's text: made once per session, never written to."""
    if key not in _ORACLE:
        want = oracle.sa(np.asarray(t))
        want.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


def _build(monkeypatch, t, env):
    """One cold build under the switches, which are taken back before it returns (a test builds many cases)."""
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, str(v))
        st = {}
        sa = sa_device(np.array(t), st, flags=_ffi.SA_COLD)
    return sa, st


def _totals(st):
    return tuple(int(st[k]) for k in M.TOTALS)


def _compare(st, w, note):
    print(note, 'build', _totals(st), 'model', w.totals())
    assert _totals(st) == w.totals(), '%s: the build reports %s = %s, the model walks\n%s' % (note, M.TOTALS, _totals(st), w)


def _key_is(st, params, note):
    got = {k: int(st[k]) for k in ('key_chars', 'key_bits', 'code_bits')}
    assert got == params, '%s: the initial key is %s, restated %s' % (note, got, params)


@pytest.mark.parametrize('name', list(M.CASES))
def test_walk_of_every_edge_case(oracle, monkeypatch, name):
    """One build per case, with the parts the model leaves out switched off and the key length forced: the oracle's suffix
    array, none of those parts taken, the initial key as restated, and the five totals equal to the model's walk."""
    case = M.CASES[name]
    t = case.text()
    sa, st = _build(monkeypatch, t, case.env())
    assert np.array_equal(sa, _want(oracle, name, t)), name
    assert all(st[k] == 0 for k in OFF), {k: st[k] for k in OFF}
    _key_is(st, M.params_of(t, case.key_chars), name)
    _compare(st, case.walk(), name)


# the variants of tests/test_sa_edges_gpu.py the model covers (all but anchor1); the first six must walk alike
TIER_VARIANTS = {
    'default': {}, 'count_sort': {'PSS_COUNT_SORT': '1'}, 'big_merge0': {'PSS_BIG_MERGE': '0'}, 'big_merge1': {'PSS_BIG_MERGE': '1'},
    'big_merge2': {'PSS_BIG_MERGE': '2'}, 'no_big_merge': {'PSS_BIG_MERGE': '1', 'PSS_NO_BIG_MERGE': '1'},
    'no_mid_tier': {'PSS_NO_MID_TIER': '1'}, 'no_mid_merge': {'PSS_NO_MID_MERGE': '1'},
    'dense': {'PSS_MODE': 'dense'}, 'sparse': {'PSS_MODE': 'sparse'}, 'text': {'PSS_MODE': 'text'},
}
_TIER_TEXTS = {}


def _tier_text(k, shape):
    if (k, shape) not in _TIER_TEXTS:
        t = np.ascontiguousarray(E.tier_case(k, shape))
        t.setflags(write=False)
        _TIER_TEXTS[k, shape] = t
    return _TIER_TEXTS[k, shape]


@pytest.mark.parametrize('variant', list(TIER_VARIANTS))
def test_walk_of_the_tier_cases(oracle, monkeypatch, variant):
    """Groups of exactly k on both sides of GS_CAP, MID_CAP and two tiles of the segmented merge, in the three shapes of
    E.tier_case: big_elems is the members of the groups beyond the tier's limit in every local round that ran, to the
    element -- and with PSS_NO_MID_MERGE the members of the groups of 513 .. 4096 in which one bin of mid_sort_kernel
    holds more than MID_KMAX.  The variants that only choose another kernel (count sort, the routes of the large groups)
    share the default's walk."""
    switches = TIER_VARIANTS[variant]
    assert (M.walk_key(switches) == M.walk_key({})) == (variant in ('default', 'count_sort', 'big_merge0', 'big_merge1', 'big_merge2', 'no_big_merge'))
    for shape in M.TIER_SHAPES:
        for k in E.TIER_KS:
            t = _tier_text(k, shape)
            note = 'tier %d %s %s' % (k, shape, variant)
            sa, st = _build(monkeypatch, t, dict(M.EXACT, PSS_KEY_CHARS=M.TIER_KEY_CHARS, **switches))
            assert np.array_equal(sa, _want(oracle, ('tier', k, shape), t)), note
            assert all(st[x] == 0 for x in OFF), note
            _key_is(st, M.params_of(t, M.TIER_KEY_CHARS), note)
            _compare(st, M.tier_walk(k, shape, switches, t), note)


def test_walk_after_the_msd_sort(oracle, monkeypatch):
    """The same texts with the MSD sort as the initial sort and its finishing kernel off: the first active list is the
    classes of the MSD sort's key (whole symbols; its length is the sort's own choice and taken from the build), and the
    same equality holds from there on.  The sort declines the texts with a group beyond its bucket."""
    took = 0
    for name, case in M.CASES.items():
        t = case.text()
        sa, st = _build(monkeypatch, t, dict(case.env(), PSS_MSD='1', PSS_MSD_NO_FINISH='1'))
        assert np.array_equal(sa, _want(oracle, name, t)), name
        assert all(st[k] == 0 for k in OFF[1:]), name
        if not st['msd']:
            # declined after the exact count, or never tried: a forced key of one radix pass carries no tie flags
            assert st['msd_max_bucket'] > E.MSD_MAX_BUCKET or case.key_chars * E.code_bits_of(t) <= 8, (name, st['msd_max_bucket'])
            continue
        took += 1
        params = {k: int(st[k]) for k in ('key_chars', 'key_bits', 'code_bits')}
        assert params['key_bits'] == params['key_chars'] * params['code_bits'] and params['code_bits'] == E.code_bits_of(t), (name, params)
        _compare(st, M.walk(t, switches=case.switches, **params), name + ' after the MSD sort')
    assert took >= len(M.CASES) - 12


def test_walk_under_the_default_switches(oracle, monkeypatch):
    """The same texts with nothing switched off (periodic keys on; the anchor round does not run below 2^20 bytes): the
    suffix array is equal, the rounds and their lists are at most the model's -- periodic keys only ever resolve more --
    and equal wherever no round used them."""
    plain = 0
    for name, case in M.CASES.items():
        t = case.text()
        sa, st = _build(monkeypatch, t, dict(case.switches, PSS_KEY_CHARS=case.key_chars))
        assert np.array_equal(sa, _want(oracle, name, t)), name
        assert st['msd'] == st['ss'] == st['rle'] == st['anchor'] == 0, name
        _key_is(st, M.params_of(t, case.key_chars), name)
        w = case.walk()
        assert st['rounds'] <= w.rounds and st['sum_active'] <= w.sum_active, (name, _totals(st), str(w))
        print(name, 'by default', _totals(st), 'model', w.totals(), 'periodic rounds', st['periodic_rounds'])
        if st['periodic_rounds'] == 0:
            plain += 1
            assert (st['rounds'], st['sum_active']) == (w.rounds, w.sum_active), '%s: the build reports %s, the model walks\n%s' % (name, _totals(st), w)
    assert plain >= len(M.CASES) // 2


@pytest.mark.parametrize('k', [513, 4097])
def test_walk_of_the_reduced_string(oracle, monkeypatch, k):
    """The run-length path sorts the string of its run symbols with the same rounds, rank rounds from depth 1, one symbol
    per key: rounds and sum_active of a PSS_RLE=1 build of R.tier_case against the walk of the string tests/rle_texts.py
    models (the sort key of every run: byte, type, length)."""
    t = np.ascontiguousarray(R.tier_case(k))
    sa, st = _build(monkeypatch, t, dict(M.EXACT, PSS_RLE='1'))
    assert np.array_equal(sa, _want(oracle, ('rle', k), t))
    assert st['rle'] != 0 and st['periodic_rounds'] == 0 and st['anchor'] == 0
    w = M.walk(R.model(t).meta, key_chars=1, key_bits=1, code_bits=1, switches={}, rank_only=True)
    print(k, (st['rounds'], st['sum_active'], st['big_elems']), str(w))
    assert (st['rounds'], st['sum_active'], st['text_rounds']) == (w.rounds, w.sum_active, 0), str(w)
