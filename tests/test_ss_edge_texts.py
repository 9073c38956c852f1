"""CPU self-checks of the sample sort's model and edge-case texts (tests/ss_edge_texts.py): every generator, at every size
the GPU tests of tests/test_ss_edges_gpu.py use, must pass the checks built into it, and the model must keep its own
invariants -- bucket sizes sum to n, no bucket below os, one sample per stratum up to the last one, the geometry of the
worked numbers in the comments of ss_sort_impl.h -- before any kernel sees a text."""
import numpy as np
import pytest

from tests import ss_edge_texts as X


def _invariants(t):
    m = X.Model(t)
    g = m.g
    assert t[-1] == X.NL
    assert int(m.sizes.sum()) == t.size and m.sizes.size == g['B1'] * g['B2']
    assert int(m.sizes.min()) >= g['os']                       # every bucket holds its own sample members
    assert np.unique(m.rank).size == t.size                    # no two elements are equal
    i = np.arange(g['S'])                                      # one sample per stratum, the last stratum included
    assert (m.pos >= i * t.size // g['S']).all() and (m.pos < (i + 1) * t.size // g['S']).all()
    # the two-level digit of the kernels, level by level, is the joint bucket
    spl1 = m.sample[g['spb']::g['spb']]
    d1 = np.searchsorted(spl1, m.rank, side='right')
    d2 = np.empty_like(d1)
    for seg in range(g['B1']):
        inside = d1 == seg
        spl2 = m.sample[seg * g['spb'] + g['st2']:(seg + 1) * g['spb']:g['st2']]
        assert spl2.size == g['B2'] - 1
        d2[inside] = np.searchsorted(spl2, m.rank[inside], side='right')
    assert np.array_equal(d1 * g['B2'] + d2, m.bucket)
    for plan in X.PLANS:
        heads = m.heads(plan)
        assert heads[0] and heads.size == m.sizes.size
        ts = m.tile_starts(plan)
        assert int(np.diff(ts).max()) <= (X.SS_TILE if plan == 'seg' else X.SS_TILE_CAP) or not m.accepted()
    return m


def test_geometry_worked_numbers():
    """The numbers the comments of ss_sort_impl.h work out, and the sizes on both sides of a change of shape."""
    g = X.geometry(1 << 29, 32)
    assert (g['B1'], g['B2'], g['os'], g['S'], g['ib'], g['kc']) == (1024, 1024, 4, 1 << 22, 29, 19)      # 19 five-bit symbols
    assert 128 - g['ib'] == 99 and g['key_bits'] == 95
    g = X.geometry(1 << 29, 29)
    assert g['kc'] == 20 and g['key_bits'] <= 99                  # 20 symbols of a 28-letter alphabet in 99 bits
    want = {1 << 16: (16, 8, 16), (1 << 16) + 1: (16, 16, 17), 1 << 20: (64, 32, 20), (1 << 20) + 1: (64, 64, 21),
            1 << 24: (256, 128, 24), 1 << 29: (1024, 1024, 29)}
    for n, (b1, b2, ib) in want.items():
        g = X.geometry(n, 29)
        assert (g['B1'], g['B2'], g['ib'], g['os'], g['S']) == (b1, b2, ib, 4, 4 * b1 * b2), n
        assert 256 <= n / (b1 * b2) <= 512 and 29 ** g['kc'] <= 1 << (128 - ib) < 29 ** (g['kc'] + 1)
    assert X.geometry((1 << 16) - 1, 29) is None and X.geometry(1 << 16, 258) is None
    assert X.geometry(1 << 20, 4)['kc'] == 32 and X.geometry(1 << 20, 2)['kc'] == 32      # never more than 32 symbols
    assert X.geometry(1 << 20, 257)['kc'] == 13
    assert X.geometry((768 << 20) + 1, 29)['os'] == 8 and X.geometry(768 << 20, 29)['os'] == 4


def test_element_by_hand():
    """b'ba\\n' with three symbols per key and two index bits: codes newline = 1, a = 2, b = 3, radix 4."""
    t = np.frombuffer(b'ba\n', dtype=np.uint8)
    g = dict(n=3, radix=4, kc=3, ib=2)
    hi, lo = X.elements(t, g)
    assert hi.tolist() == [0, 0, 0]
    assert lo.tolist() == [((3 * 16 + 2 * 4 + 1) << 2) | 0, ((2 * 16 + 1 * 4) << 2) | 1, ((1 * 16) << 2) | 2]
    # all 256 byte values: raw bytes + 1 in base 257
    t = np.arange(256, dtype=np.uint8)
    hi, lo = X.elements(t, dict(n=256, radix=257, kc=2, ib=8))
    assert lo[0] == ((1 * 257 + 2) << 8) and lo[255] == ((256 * 257) << 8 | 255)
    # a key that fills the high word: 13 symbols of base 257, 17 index bits
    t = np.full(70000, 255, np.uint8)
    t[:256] = np.arange(256)
    g = X.geometry(70000, 257)
    hi, lo = X.elements(t, g)
    number = ((257 ** 13 - 1) << 17) | 300                      # thirteen times the largest code, 256
    assert ((int(hi[300]) << 64) | int(lo[300])) == number


def test_sample_positions():
    for n in (1 << 16, (1 << 16) + 1, 70001, (1 << 20) + 4097):
        g = X.geometry(n, 29)
        pos = X.sample_positions(n, g['S'])
        i = np.arange(g['S'])
        assert (pos >= i * n // g['S']).all() and (pos < (i + 1) * n // g['S']).all()
    # the hash itself, worked by hand for i = 0 at n = 2^16 (strata of 128 bytes)
    x = 0x9E3779B97F4A7C15
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x ^= x >> 32
    assert X.sample_positions(1 << 16, 512)[0] == x % 128


def test_plans_by_hand():
    # greedy: the longest run that fits
    assert X.heads_greedy(np.array([2048, 2048, 8, 4088, 8, 8]), 4096).tolist() == [True, False, True, False, True, False]
    assert X.heads_greedy(np.array([2044, 2044, 1, 4088, 1]), 4088).tolist() == [True, False, True, True, True]
    # window rule, windows of 10 slots and a cap of 12: the buckets that start inside a window share a tile unless they
    # hold more than the cap together, then the window's last bucket goes alone
    assert X.heads_window(np.array([4, 4, 4, 4, 9, 1]), 10, 12).tolist() == [True, False, False, True, True, True]
    assert X.heads_window(np.array([4, 4, 5, 4]), 10, 12).tolist() == [True, False, True, True]


@pytest.mark.parametrize('k', X.BUCKET_KS)
def test_bucket_cases(k):
    m = _invariants(X.bucket_case(k))
    assert int(m.sizes.max()) == k and m.accepted() == (k <= 4088) and (1 << 16) <= m.n <= (1 << 18)


def test_packed_cases():
    for name, (sizes, want) in X.PACKED.items():
        m = _invariants(X.packed_case(name))
        assert tuple(m.sizes[-len(sizes):]) == sizes and m.n % 16
        for plan in ('seg', 'tile'):
            assert tuple(m.heads(plan)[-len(sizes) + 1:].astype(int)) == want[plan]
    # what the planted buckets add to the difference between the two greedy plans
    assert {name: sum(w['seg']) - sum(w['tile']) for name, (_, w) in X.PACKED.items()} == \
        {'pad4096': -1, 'pad4104': 1, 'plain4088': 0, 'plain4089': -1, 'full_small': -1, 'big_small': 0}


def test_segments_case():
    m = _invariants(X.segments_case())
    assert 290000 <= m.n <= 310000 and m.n % 16


def test_settle_and_shift_cases():
    seen = set()
    for want in X.SETTLE_MS:
        m = _invariants(X.settle_case(want))
        steps = m.settle_steps()
        assert int(steps.max()) == want
        seen |= set(m.cell_shifts())
    assert min(X.SETTLE_MS) == 1 and {7, 8, 9} <= set(X.SETTLE_MS) and max(X.SETTLE_MS) >= 12
    for name in ('two', 'all'):
        seen |= set(_invariants(X.shift_case(name)).cell_shifts())
    assert 0 in seen and 64 in seen and any(0 < s < 64 for s in seen) and any(s > 64 for s in seen)


def test_ties_case():
    m = _invariants(X.ties_case())
    for plan in X.PLANS:
        inner, outer = m.groups_cut(plan)
        assert inner and outer
        # direct suffix comparison: across each border, text order differs from index order
        for s, a, b in inner + outer:
            left = m.order[a:s]
            group = sorted(m.order[a:b], key=lambda i: m.t[i:].tobytes())
            assert set(group[:s - a]) != set(left.tolist()), (plan, s, a, b)
        assert len(m.tied_heads(plan)) == len(outer)


@pytest.mark.parametrize('wide', [False, True])
def test_tail_cases(wide):
    for d in X.TAIL_DS:
        m = _invariants(X.tail_case(d, wide))
        assert m.n % 16 and m.g['radix'] == (257 if wide else 41)
        if not wide:
            assert m.pos[-1] >= m.n - m.g['kc']


def test_unplanted_and_device_sorted_cases():
    for name in X.UNPLANTED:
        m = _invariants(X.unplanted_case(name))
        assert m.accepted() and (1 << 16) <= m.n <= (1 << 18)
    for name in ('two', 'all'):
        m = _invariants(X.device_sorted_case(name))
        assert m.accepted() and m.g['S'] > X.HOST_SORT_MAX
