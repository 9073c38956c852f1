"""The two partition passes of the MSD sort stage a whole 16384-element tile in LDS at once, and the first pass asks for the
code words of a range's next tile while it writes the current one out (msd_scatter2_kernel, msd_scatter_lb_kernel in
msd_sort.hip).  The texts of tests/scatter_tile_texts.py put the passes on every edge of that: a short tile whose upper
half is never staged, ranges of exactly one tile (nothing to load ahead), of a tile and a half (the words loaded ahead
belong to a half tile, the text ends 1 / 7 / 16 / 8191 elements into it), of several tiles, and d-regions of the second
pass of 0, 1, 8191, 8192, 8193 and 16383 elements mod 16384.  Every suffix array is compared with the oracle's, in LSD
order (the default: first pass + look-back pass) and in MSD order (PSS_MSD_LSD=0: both passes by msd_scatter2_kernel).

Measured on one MI355X: the sixteen cases take 6.5 s together; the slowest is 0.95 s (`several`, 24 MiB: generator,
libsais and the sort; whichever case runs first adds the second and a half of starting the device), a case in the second
order reuses text and oracle and takes 0.02 s."""
import numpy as np
import pytest

from tests import scatter_tile_texts as S
from tests.util import sa_device

pytestmark = pytest.mark.gpu

ORDERS = {'lsd': None, 'msd_order': '0'}
_CACHE = {}


def _case(oracle, name):
    """(text, the oracle's suffix array): made once per session, never written to."""
    if name not in _CACHE:
        t = np.ascontiguousarray(S.CASES[name]())
        want = oracle.sa(t)
        want.setflags(write=False)
        t.setflags(write=False)
        _CACHE[name] = (t, want)
    return _CACHE[name]


@pytest.mark.parametrize('order', list(ORDERS))
@pytest.mark.parametrize('name', list(S.CASES))
def test_tiles_of_both_passes(oracle, monkeypatch, name, order):
    monkeypatch.setenv('PSS_MSD', '1')
    monkeypatch.setenv('PSS_PERIOD', '0')
    monkeypatch.delenv('PSS_MSD_LSD', raising=False)
    if ORDERS[order] is not None:
        monkeypatch.setenv('PSS_MSD_LSD', ORDERS[order])
    t, want = _case(oracle, name)
    st = {}
    sa = sa_device(np.array(t), st)                      # (a writable copy: the text itself is shared between the orders)
    note = (name, order)
    print(note, {k: st[k] for k in ('msd', 'msd_tiles', 'msd_max_bucket', 'code_bits', 'key_chars', 'key_bits')})
    assert np.array_equal(sa, want), note
    assert st['msd'] == 1, note
