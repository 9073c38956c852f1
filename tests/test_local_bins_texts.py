"""Every generator of tests/local_bins_texts.py, on the CPU: each asserts the geometry its GPU test relies on."""
import numpy as np
import pytest

from tests import local_bins_texts as B
from tests import local_rows_texts as L


@pytest.mark.parametrize('name', list(B.TEXTS))
def test_text(name):
    t = B.TEXTS[name]()
    assert t.dtype == np.uint8 and t[-1] == 10 and t.size < 1 << 18
    assert len(B.Plan(t).slow_tiles()) == B.SLOW_TILES[name]


@pytest.mark.parametrize('cap', B.WIDTH_CAPS)
def test_widths(cap):
    t, p = B.widths_case(cap)
    assert p.slow_tiles() == []
    t2, q = B.widths_case(cap, lsd=False)
    assert np.array_equal(t, t2) and q.slow_tiles() == []
    B.widths_cover()


def test_plan_restates_view():
    """Plan and local_rows_texts.View describe the default format alike, on a text of that file with a declined tile."""
    t = L.decline_case()
    v, p = L.View(t), B.Plan(t)
    assert np.array_equal(v.e0, p.e0) and np.array_equal(v.counts, p.counts) and np.array_equal(v.keys, p.keys)
    assert v.slow_tiles() == p.slow_tiles() and len(p.slow_tiles()) == 1


def test_window_matches_kernel():
    """LS_WINDOW, LS_BIN_BITS and LS_DECLINE_BITS of msd_sort.hip are the ones the cases are built around."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), '..', 'pysubstringsearch_amd', 'csrc', 'msd_sort.hip')).read()
    assert int(re.search(r'#define PSS_LS_WINDOW (\d+)', src).group(1)) == B.LS_WINDOW
    assert int(re.search(r'#define PSS_LS_BIN_BITS (\d+)', src).group(1)) == B.BIN_BITS
    assert int(re.search(r'LS_DECLINE_BITS = (\d+)', src).group(1)) == B.DECLINE_BITS
