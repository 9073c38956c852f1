"""msd_local_fast_kernel (msd_sort.hip) counts a tile into 8192 bins held in ONE array of 16-bit counters: counts, then
starts, then -- after the slot atomics -- ends, the start of bin b being read from entry b - 1; every element ranks itself
in a window of LS_WINDOW members of its bin and a longer bin finishes in a loop; a tile is declined when more than LS_KMAX
elements share the top 12 bits (a pair of bins).  The texts of tests/local_bins_texts.py put tiles on every edge of that:
pairs of 64 and 65 split over their halves, the first and the last bin, a tile with nothing between them, bins of
LS_WINDOW and LS_WINDOW + 1 members in a tail row, a full row and across a row border, a bin between long runs of empty
ones, keys of 10 .. 16 bits in tiles of one, two and three buckets, and counters that end at 8176.  Each generator
asserts its geometry on the CPU; every suffix array is compared with the oracle's, the statistics with the models, in
LSD and in MSD digit order."""
import numpy as np
import pytest

from tests import local_bins_texts as B
from tests import msd_finish_texts as F
from tests.util import sa_device

pytestmark = pytest.mark.gpu

ORDERS = {'lsd_order': True, 'msd_order': False}
_CACHE = {}


def _text(oracle, name, make):
    """(text, the oracle's suffix array): made once per session, never written to."""
    if name not in _CACHE:
        t = np.ascontiguousarray(make())
        want = oracle.sa(t)
        want.setflags(write=False)
        t.setflags(write=False)
        _CACHE[name] = (t, want)
    return _CACHE[name]


def _plan(name, t, lsd, **fmt):
    k = ('plan', name, lsd, tuple(sorted(fmt.items())))
    if k not in _CACHE:
        p = B.Plan(t, lsd=lsd, **fmt)
        _CACHE[k] = (p, F.Model(t, p.f))
    return _CACHE[k]


def _build_and_check(monkeypatch, t, want, p, m, lsd, note):
    monkeypatch.setenv('PSS_MSD', '1')
    monkeypatch.setenv('PSS_PERIOD', '0')
    monkeypatch.setenv('PSS_MSD_LSD', '1' if lsd else '0')
    st = {}
    sa = sa_device(np.array(t), st)                      # (a writable copy: the text itself is shared)
    print(note, {k: st[k] for k in ('msd', 'msd_tiles', 'msd_slow_tiles', 'msd_finished', 'sum_active', 'rounds')},
          'model tiles', len(p.e0), 'slow', p.slow_tiles(), 'finished', m.n_finished, 'left', m.n_left)
    assert np.array_equal(sa, want), note
    assert st['msd'] == 1 and st['rle'] == 0 and st['period_path'] == 0, note
    assert (st['code_bits'], st['key_chars'], st['key_bits']) == (p.f.b, p.f.kc, p.f.kb), note
    assert st['msd_tiles'] == len(p.e0), note
    assert st['msd_slow_tiles'] == len(p.slow_tiles()), note
    assert st['msd_finished'] == m.n_finished, note
    assert st['sum_active'] >= m.n_left and (st['sum_active'] > 0) == (m.n_left > 0), note
    assert (st['rounds'] > 0) == (st['sum_active'] > 0), note      # (rounds run exactly when the sort left records)
    return st


@pytest.mark.parametrize('order', list(ORDERS))
@pytest.mark.parametrize('name', list(B.TEXTS))
def test_bins(oracle, monkeypatch, name, order):
    t, want = _text(oracle, name, B.TEXTS[name])
    lsd = ORDERS[order]
    p, m = _plan(name, t, lsd)
    st = _build_and_check(monkeypatch, t, want, p, m, lsd, (name, order))
    if lsd:                                              # (the cases are built on the default plan)
        assert st['msd_slow_tiles'] == B.SLOW_TILES[name], (name, order)


@pytest.mark.parametrize('order', list(ORDERS))
@pytest.mark.parametrize('cap', B.WIDTH_CAPS)
def test_key_widths(oracle, monkeypatch, cap, order):
    """Tiles of one, two and three buckets whose keys are cap - 20, + 1 and + 2 bits wide: on both sides of the 13 bin bits
    and of the 12 bits of the decline rule (where the key is narrower than either, the bins are the keys)."""
    monkeypatch.setenv('PSS_MSD_KEY_CAP', str(cap))
    monkeypatch.setenv('PSS_MSD_PARTIAL_SYMBOL', '1')
    t, want = _text(oracle, 'widths', B.widths_text)
    lsd = ORDERS[order]
    B.widths_case(cap, lsd)
    p, m = _plan('widths', t, lsd, cap=cap, partial=True)
    _build_and_check(monkeypatch, t, want, p, m, lsd, ('widths', cap, order))
