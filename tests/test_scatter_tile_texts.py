"""Every generator of tests/scatter_tile_texts.py runs on the CPU: the asserts inside them are the proof that a text puts
the partition passes on the tile edges its case is about."""
import numpy as np
import pytest

from tests import sa_edge_texts as E
from tests import scatter_tile_texts as S

SIZES = {'short5000': 5000, 'short8193': 8193, 'full': (1 << 23) + 2 * 8192, 'several': 3 * (1 << 23) + 8192 + 5,
         **{f'half{d}': (1 << 24) + 3 * 8192 + d for d in S.HALF_DS}}
TILES_PER_RANGE1 = {'short5000': 1, 'short8193': 1, 'full': 2, 'several': 4, **{f'half{d}': 3 for d in S.HALF_DS}}


@pytest.mark.parametrize('name', list(S.CASES))
def test_case_is_what_it_says(name):
    t = S.CASES[name]()
    assert t.dtype == np.uint8 and t.size == SIZES[name] and t[-1] == E.NL
    assert set(np.flatnonzero(np.bincount(t, minlength=256))) == set(S.SYMS)      # the 39 symbols: 6-bit codes
    assert S.Geometry(t.size).tiles_per_range1 == TILES_PER_RANGE1[name]
    if t.size < (1 << 20):
        assert np.array_equal(t, S.CASES[name]())   # the same text on every call


def test_steering_is_seeded_and_exact():
    """A small text steered to residues of a small modulus' worth: the same text on every call, the sizes as asked."""
    want = None
    texts = []
    for _ in range(2):
        t = S.lines(1 << 18, 77)
        regions = S.pick_regions(t, 78, 3)
        size = S.region_sizes(t)
        want = {d: (int(size[d]) + delta) % S.TILE2 for d, delta in zip(regions, (-40, 1, 25))}
        S.steer(t, 79, want)
        texts.append(t)
    assert np.array_equal(texts[0], texts[1])
    size = S.region_sizes(texts[0])
    assert all(int(size[d]) % S.TILE2 == r for d, r in want.items())
    assert (S.joint(texts[0]) == E.joint_buckets(texts[0], S.B)).all()


def test_geometry_matches_the_issue_table():
    g = S.Geometry((1 << 24) + 3 * 8192 + 7)
    assert (g.tiles_per_range1, g.tiles_of(0)) == (3, [(0, 16384), (16384, 8192)])
    assert S.Geometry(8 << 20).tiles_per_range1 == 1 and not S.Geometry(8 << 20).ahead_carries()
