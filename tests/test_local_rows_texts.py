"""Every generator of tests/local_rows_texts.py runs on the CPU: the asserts inside them are the proof that a text holds
the tiles, ties and bins its case is about."""
import numpy as np
import pytest

from tests import local_rows_texts as L
from tests import sa_edge_texts as E


@pytest.mark.parametrize('name', list(L.CASES))
def test_case_is_what_it_says(name):
    t = L.CASES[name]()
    assert t.dtype == np.uint8 and (1 << 17) <= t.size <= (1 << 18) and t[-1] == E.NL
    assert E.code_bits_of(t) == 7
    u = L.CASES[name]()
    assert np.array_equal(t, u)                      # the same text on every call


def test_msd_order_plans_the_same_lone_tiles():
    """PSS_MSD_LSD=0 packs tiles by blocks of 2048 non-empty buckets: the plan differs, its tile count is the model's."""
    t = L.CASES['counts']()
    assert E.tile_count(t, lsd=False) >= 1 and E.tile_count(t, lsd=True) >= len(L.COUNT_TILES)
