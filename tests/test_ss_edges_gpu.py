"""The sample sort on its limits (ss_sort_impl.h, ss_suffix_sort): joint buckets against the tile (SS_MAX_BUCKET 4088), tiles
packed to the last slot under the three plans (padded lengths against SS_TILE 4096, plain lengths against SS_TILE_CAP
4088, the window rule), more segments of the greedy plan than one jump table covers, first-level splitters that share a
high word (the walk and the bisection of ss_settle), every shift case of ss_cell_of, groups of equal keys across bucket and
tile borders (ss_boundary_kernel), keys that run past the end of the text.

Suffix-array equality cannot see a sampler that draws from the wrong strata, a mis-sorted sample or a plan that packs
badly -- any splitters give the exact result -- so every accepted build is also held to the CPU model of
tests/ss_edge_texts.py: ss_buckets, ss_max_bucket, ss_samples and ss_tiles must be the model's numbers for that plan.
Whether a text reaches a branch is established by the model on the text (tests/test_ss_edge_texts.py runs those checks
without a GPU).  Every suffix array is compared with the oracle's for equality: it is unique, there is no tolerance."""
import numpy as np
import pytest

from tests import ss_edge_texts as X
from tests.util import sa_device

pytestmark = pytest.mark.gpu

_CACHE = {}
MODES = (None, 'dense', 'text')


def _case(oracle, key, make):
    """(text, the oracle's suffix array, the model): made once per session, never written to."""
    if key not in _CACHE:
        t = np.ascontiguousarray(make())
        want = oracle.sa(t)
        want.setflags(write=False)
        _CACHE[key] = (t, want, X.Model(t))
    return _CACHE[key]


def _build(monkeypatch, case, plan, mode=None, note=None):
    """One forced build under the plan: the oracle's bytes, no shortcut taken, and the model's statistics."""
    t, want, m = case
    for k, v in dict(PSS_SS=1, PSS_MSD=0, PSS_RLE=0, PSS_PERIOD=0).items():
        monkeypatch.setenv(k, str(v))
    for k in ('PSS_SS_SEG', 'PSS_SS_WINDOW_PLAN', 'PSS_MODE'):
        monkeypatch.delenv(k, raising=False)
    for k, v in X.PLAN_ENV[plan].items():
        monkeypatch.setenv(k, v)
    if mode:
        monkeypatch.setenv('PSS_MODE', mode)
    st = {}
    sa = sa_device(np.asarray(t), st)
    note = (note, plan, mode)
    assert np.array_equal(sa, want), note
    assert st['rle'] == 0 and st['period_path'] == 0, note
    model = m.stats(plan)
    got = {k: int(st[k]) for k in model}
    print(note, 'ss', st['ss'], 'build', got, 'model', model)
    assert st['ss'] == (1 if m.accepted() else 0), note
    if not m.accepted():
        model['ss_tiles'] = 0                      # the statistics are filled before the sort declines, the plan is not made
    assert got == model, note
    return st


# ---- a. bucket against the tile --------------------------------------------------------------------------------------

@pytest.mark.parametrize('plan', X.PLANS)
@pytest.mark.parametrize('k', X.BUCKET_KS)
def test_bucket_of_exactly_k_against_the_tile(oracle, monkeypatch, k, plan):
    """One joint bucket of exactly k elements behind the last splitter, no other above 4087: the sort takes 4087 and 4088
    and declines 4089 and 4090 after the count -- the build falls back and still gives libsais' bytes."""
    case = _case(oracle, ('bucket', k), lambda: X.bucket_case(k))
    st = _build(monkeypatch, case, plan, note=k)
    assert st['ss_max_bucket'] == k
    assert st['ss'] == (1 if k <= X.SS_MAX_BUCKET else 0)


# ---- b, c. tile plans ------------------------------------------------------------------------------------------------

def test_tiles_packed_to_the_last_slot(oracle, monkeypatch):
    """Adjacent buckets whose padded lengths sum to 4096 and 4104, whose plain lengths sum to 4088 and 4089, and a bucket
    of 4088 / 4081 next to one of 5 / 7 (X.PACKED): each plan gives the model's number of tiles, and the two greedy plans
    differ on the planted buckets by what the sums say (the rest of a text is random, its share comes from the model)."""
    for name, (sizes, want) in X.PACKED.items():
        case = _case(oracle, ('packed', name), lambda: X.packed_case(name))
        m = case[2]
        tiles = {plan: _build(monkeypatch, case, plan, note=name)['ss_tiles'] for plan in X.PLANS}
        for a in X.PLANS:
            for b in X.PLANS:
                assert tiles[a] - tiles[b] == int(m.heads(a).sum()) - int(m.heads(b).sum()), (name, a, b)
        ahead = len(m.sizes) - len(sizes) + 1             # buckets before the planted ones (the guard included)
        rest = int(m.heads('seg')[:ahead].sum()) - int(m.heads('tile')[:ahead].sum())
        assert tiles['seg'] - tiles['tile'] == rest + sum(want['seg']) - sum(want['tile']), name


@pytest.mark.parametrize('plan', X.PLANS)
def test_many_segments_of_the_greedy_plan(oracle, monkeypatch, plan):
    """300 007 bytes of word-like text: five segments of SS_PLAN_SEG slots (three levels of jump tables), a tile across a
    segment's end: the chain that is put together from the segments must be the chain walked in one piece."""
    _build(monkeypatch, _case(oracle, ('segments',), X.segments_case), plan)


# ---- d. equal high words, shift cases --------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('plan', X.PLANS)
def test_splitters_that_share_a_high_word(oracle, monkeypatch, plan, mode):
    """A run of one byte under PSS_RLE=0: 1, 7, 8, 9 and 13 first-level splitters share the high word of elements below
    them -- ss_settle walks up to eight steps and bisects the rest -- and the first-level buckets inside the run have
    second-level splitters that differ in their index bits alone (csh == 0).  A search that stops at the high words still
    cuts the elements monotonically, so it gives the right bytes: it shows in ss_buckets and ss_max_bucket (the buckets
    between the splitters of one high word come out empty, the one behind them holds them all)."""
    for steps in X.SETTLE_MS:
        _build(monkeypatch, _case(oracle, ('settle', steps), lambda: X.settle_case(steps)), plan, mode, note=steps)


@pytest.mark.parametrize('plan', X.PLANS)
def test_every_shift_case_of_the_cell_table(oracle, monkeypatch, plan):
    """Two-letter text (0 < csh < 64, csh == 64, csh > 64 inside one build) and all 256 byte values (csh > 100)."""
    for name in ('two', 'all'):
        _build(monkeypatch, _case(oracle, ('shift', name), lambda: X.shift_case(name)), plan, note=name)


# ---- e. ties across borders ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('plan', X.PLANS)
def test_equal_keys_across_bucket_and_tile_borders(oracle, monkeypatch, plan, mode):
    """Groups of 100 elements with equal key bits, cut by bucket borders inside a tile (the flag comes from the last element
    of the bucket before) and by tile borders (ss_boundary_kernel).  In every such group libsais' order across the border
    differs from index order, so a missing flag -- two halves ranked apart -- cannot give the right bytes."""
    case = _case(oracle, ('ties',), X.ties_case)
    t, want, m = case
    inner, outer = m.groups_cut(plan)
    assert inner and outer
    for s, a, b in inner + outer:
        assert set(want[a:b].tolist()) == set(m.order[a:b].tolist())
        assert set(want[a:s].tolist()) != set(m.order[a:s].tolist()), (plan, s, a, b)
    _build(monkeypatch, case, plan, mode)


# ---- f. the end of the text ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('plan', X.PLANS)
@pytest.mark.parametrize('wide', [False, True])
def test_word_at_the_tail_of_the_text(oracle, monkeypatch, wide, plan):
    """The last copy of a word ends 0, 1, 7, 8, 15, 16 bytes before the final newline, lengths no multiple of 16, over 39
    symbols (with a sample inside the last kc bytes) and over all 256 byte values (raw bytes + 1: the packers tell the end
    of the text by the index)."""
    for d in X.TAIL_DS:
        _build(monkeypatch, _case(oracle, ('tail', d, wide), lambda: X.tail_case(d, wide)), plan, note=(d, wide))


# ---- the model on texts nothing is planted in ------------------------------------------------------------------------

@pytest.mark.parametrize('plan', X.PLANS)
def test_model_matches_on_unplanted_texts(oracle, monkeypatch, plan):
    for name in X.UNPLANTED:
        st = _build(monkeypatch, _case(oracle, ('unplanted', name), lambda: X.unplanted_case(name)), plan, note=name)
        assert st['ss'] == 1


@pytest.mark.parametrize('plan', X.PLANS)
@pytest.mark.parametrize('name', ['two', 'all'])
def test_model_matches_with_the_sample_sorted_on_the_device(oracle, monkeypatch, name, plan):
    """2^20 + 4097 bytes and a little more: 16 384 samples, sorted by the two chained device radix sorts (21 and 62 bits of
    the high word).  A sample that came back out of order would move splitters, hence bucket sizes and tiles."""
    st = _build(monkeypatch, _case(oracle, ('device_sorted', name), lambda: X.device_sorted_case(name)), plan, note=name)
    assert st['ss'] == 1 and st['ss_samples'] == 16384
