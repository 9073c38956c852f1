"""msd_local_fast_kernel (msd_sort.hip) runs the full rows of a tile without a lane predicate and one predicated tail row,
and writes the records of tied elements in a loop behind the rows.  The texts of tests/local_rows_texts.py put tiles on
every edge of that structure -- counts of 1, 511, 512, 513, 1024, 1025, MSD_TILE_CAP, a lone bucket of MSD_MAX_BUCKET;
ties across a row border, in the first and the last slots of a tile, next to an equal key of the next tile, in several
rows of one thread; bins of 8, 9, 64 and 65 members in the tail row -- and a CPU-side assert in each generator checks that
the text holds them.  Every suffix array is compared with the oracle's for equality, the statistics with the models."""
import numpy as np
import pytest

from tests import local_rows_texts as L
from tests import sa_edge_texts as E
from tests.util import sa_device

pytestmark = pytest.mark.gpu

ROUTES = {'default': {}, 'no_fuse': {'PSS_MSD_NO_FUSE': '1'}, 'no_finish': {'PSS_MSD_NO_FINISH': '1'},
          'msd_order': {'PSS_MSD_LSD': '0'}}
_CACHE = {}


def _case(oracle, name):
    """(text, the oracle's suffix array, the model under the default plan): made once per session, never written to."""
    if name not in _CACHE:
        t = np.ascontiguousarray(L.CASES[name]())
        want = oracle.sa(t)
        v = L.View(t)
        want.setflags(write=False)
        t.setflags(write=False)
        _CACHE[name] = (t, want, v)
    return _CACHE[name]


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('name', list(L.CASES))
def test_rows_and_records(oracle, monkeypatch, name, route):
    monkeypatch.setenv('PSS_MSD', '1')
    monkeypatch.setenv('PSS_PERIOD', '0')
    for k, val in ROUTES[route].items():
        monkeypatch.setenv(k, val)
    t, want, v = _case(oracle, name)
    st = {}
    sa = sa_device(np.array(t), st)                      # (a writable copy: the text itself is shared between the routes)
    note = (name, route)
    print(note, {k: st[k] for k in ('msd', 'msd_tiles', 'msd_slow_tiles', 'msd_finished', 'sum_active', 'rounds')},
          'model tiles', E.tile_count(t, route != 'msd_order'), 'finished', v.m.n_finished, 'left', v.m.n_left)
    assert np.array_equal(sa, want), note
    assert st['msd'] == 1 and st['rle'] == 0 and st['period_path'] == 0, note
    assert (st['code_bits'], st['key_chars'], st['key_bits']) == (v.f.b, v.f.kc, v.f.kb), note
    assert st['msd_tiles'] == E.tile_count(t, route != 'msd_order'), note
    if route != 'msd_order':                             # (another plan: the bin of 65 need not be alone in its tile's top bits)
        assert st['msd_slow_tiles'] == L.SLOW_TILES[name], note
    # the finish model (tests/msd_finish_texts.py): ties are groups under the key, whatever the plan
    if route in ('default', 'msd_order'):
        assert st['msd_finished'] == v.m.n_finished, note
        assert st['sum_active'] >= v.m.n_left and (st['sum_active'] > 0) == (v.m.n_left > 0), note
    else:
        assert st['msd_finished'] == 0, note
        assert st['sum_active'] >= v.m.n_left + v.m.n_finished, note
