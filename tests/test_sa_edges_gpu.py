"""The builder's kernels on their limits: joint buckets against the local-sort tile (msd_sort.hip: MSD_MAX_BUCKET 4088,
MSD_TILE_CAP 8176, MSD_WIN 6144), bins of the fast local sort (LS_WINDOW 8, LS_KMAX 64), tag blocks (64 joint buckets in
LSD order, 2048 non-empty ones in MSD order), the group-size tiers of the rounds (sa_rounds_impl.h: GS_CAP 512, MID_CAP
4096, MID_KMAX 512, BG_TILE 4096), and every builder switch that no other test sets.  The texts come from
tests/sa_edge_texts.py, which checks on the CPU that they hold what a case is about; every suffix array is compared
with the oracle's for equality -- it is unique, so there is no tolerance anywhere."""
import hashlib

import numpy as np
import pytest

from tests import rounds_model as M
from tests import sa_edge_texts as E
from tests.util import gen_corpus, sa_device

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(oracle, key, make):
    """(text, the oracle's suffix array): made once per session, never written to."""
    if key not in _CACHE:
        t = np.ascontiguousarray(make())
        want = oracle.sa(t)
        want.setflags(write=False)
        _CACHE[key] = (t, want)
    return _CACHE[key]


def _build(t, want, note=None):
    st = {}
    sa = sa_device(np.asarray(t), st)
    assert np.array_equal(sa, want), note
    assert st['rle'] == 0 and st['period_path'] == 0, note          # the sort and the rounds made this suffix array
    return st


def _env(monkeypatch, **kv):
    for k, v in kv.items():
        monkeypatch.setenv(k, str(v))


ORDERS = {'lsd': {}, 'msd_order': {'PSS_MSD_LSD': '0'}, 'slow_local': {'PSS_MSD_SLOW_LOCAL': '1'}}


# ---- 2. MSD sort: bucket and tile capacity ---------------------------------------------------------------------------

@pytest.mark.parametrize('order', ['lsd', 'msd_order', 'slow_local'])
@pytest.mark.parametrize('k', E.BUCKET_KS)
def test_bucket_of_exactly_k_against_the_tile(oracle, monkeypatch, k, order):
    """One joint bucket of exactly k suffixes (and one more of k at every position of the planted word): the path takes
    4087 and 4088, and declines 4089, 4090, 8176, 8177 after the exact count -- the LSD passes then give the same bytes.
    msd_lookback says which order the two digits took (it is only filled when the path ran)."""
    _env(monkeypatch, PSS_MSD=1, PSS_PERIOD=0, **ORDERS[order])
    t, want = _case(oracle, ('bucket', k), lambda: E.bucket_case(k))
    st = _build(t, want, (k, order))
    assert st['msd_max_bucket'] == k
    assert st['msd'] == (1 if k <= E.MSD_MAX_BUCKET else 0)
    assert st['msd_lookback'] == (1 if k <= E.MSD_MAX_BUCKET and order != 'msd_order' else 0)


@pytest.mark.parametrize('order', ['lsd', 'msd_order', 'slow_local'])
def test_tiles_packed_to_the_last_slot(oracle, monkeypatch, order):
    """Large buckets next to each other (E.tile_case): 4088 + 4088 from the start of a window is one tile of exactly
    MSD_TILE_CAP elements, one element more in front of them splits it; a run of buckets that start inside one window and
    hold more than a tile sends the window's last bucket off alone; 4088 after 4088 after 4088.  The number of tiles is
    the one the restated rule (E.tile_heads) plans, and differs by one between the pair and the trio."""
    _env(monkeypatch, PSS_MSD=1, PSS_PERIOD=0, **ORDERS[order])
    tiles = {}
    for name in ('pair8176', 'trio8177', 'run', 'chain'):
        t, want = _case(oracle, ('tile', name), lambda: E.tile_case(name))
        st = _build(t, want, (name, order))
        sizes = E.bucket_sizes(t)[1]
        assert st['msd'] == 1 and st['msd_max_bucket'] == int(sizes.max()) and st['msd_buckets'] == len(sizes), name
        tiles[name] = st['msd_tiles']
        print(name, order, 'tiles', st['msd_tiles'], 'model', E.tile_count(t, order != 'msd_order'))
        assert st['msd_tiles'] == E.tile_count(t, order != 'msd_order'), name
    assert tiles['trio8177'] - tiles['pair8176'] == 1


@pytest.mark.parametrize('order', ['lsd', 'msd_order'])
def test_joint_bucket_model_matches_the_histogram_passes(oracle, monkeypatch, order):
    """The numpy model of a suffix's joint bucket (dense codes, big-endian packing, top 20 bits of the key) against the
    bucket count and the largest bucket the histogram passes report, on three random texts of different code widths."""
    _env(monkeypatch, PSS_MSD=1, PSS_PERIOD=0, **ORDERS[order])
    rng = np.random.default_rng(31)
    for alpha, n in ((4, 70001), (39, (1 << 18) + 3), (200, 300007)):
        t, want = _case(oracle, ('random', alpha), lambda: np.append(rng.integers(40, 40 + alpha, n - 1).astype(np.uint8), np.uint8(10)))
        st = _build(t, want, alpha)
        assert st['msd'] == 1
        j = E.joint_buckets(t, st['code_bits'], st['key_chars'], st['key_bits'])
        numbers, sizes = np.unique(j, return_counts=True)
        assert (st['msd_buckets'], st['msd_max_bucket']) == (len(sizes), int(sizes.max())), alpha
        assert np.array_equal(numbers, E.bucket_sizes(t)[0])
        assert st['msd_tiles'] == int(E.tile_heads(numbers, sizes, t.size, order == 'lsd').sum()), alpha


@pytest.mark.parametrize('order', ['lsd', 'msd_order'])
def test_tiny_buckets_across_tag_blocks(oracle, monkeypatch, order):
    """Thousands of tiny non-empty buckets in a row (more than a tag block holds inside every window), without and with
    one bucket of 3000 sitting exactly on a block boundary: a multiple of 64 joint buckets in LSD order, the 2048th
    non-empty bucket times 43 in MSD order.  Both texts in both orders (a text made for one order is just a text in the other)."""
    _env(monkeypatch, PSS_MSD=1, PSS_PERIOD=0, **ORDERS[order])
    for made_for in (True, False):
        for big in (False, True):
            t, want = _case(oracle, ('tag', big, made_for), lambda: E.tagblock_case(big, made_for))
            st = _build(t, want, (big, made_for, order))
            numbers, sizes = E.bucket_sizes(t)
            assert st['msd'] == 1 and st['msd_buckets'] == len(sizes) and st['msd_max_bucket'] == int(sizes.max())
            assert st['msd_tiles'] == int(E.tile_heads(numbers, sizes, t.size, order == 'lsd').sum()), (big, made_for)


# ---- 3. MSD local sort: bin occupancy --------------------------------------------------------------------------------

LOCAL_VARIANTS = {'default': {}, 'no_fuse': {'PSS_MSD_NO_FUSE': '1'}, 'partial_symbol': {'PSS_MSD_PARTIAL_SYMBOL': '1'},
                  'msd_order_scatter': {'PSS_MSD_LSD': '0', 'PSS_MSD_SCATTER': '1'}}


@pytest.mark.parametrize('variant', list(LOCAL_VARIANTS))
def test_bins_of_exactly_k_equal_keys(oracle, monkeypatch, variant):
    """Every position of the planted word is a run of k equal keys in one bin of the local sort: k on both sides of
    LS_WINDOW = 8 and LS_KMAX = 64.  From 65 on the fast kernel must hand the tile over (equal keys share a bin); below,
    a stray neighbour may share the bin, so nothing is claimed.  6-bit and 7-bit codes (PSS_MSD_PARTIAL_SYMBOL changes the
    key of the latter: 6 symbols + 6 bits of the 7th).  Ties emitted from the local sort, or flagged (PSS_MSD_NO_FUSE)."""
    _env(monkeypatch, PSS_MSD=1, **LOCAL_VARIANTS[variant])
    for wide in (False, True):
        for k in E.BIN_KS:
            t, want = _case(oracle, ('bin', k, wide), lambda: E.bin_case(k, wide))
            st = _build(t, want, (k, wide, variant))
            assert st['msd'] == 1 and st['msd_lookback'] == (0 if variant == 'msd_order_scatter' else 1)
            if k > E.LS_KMAX:
                assert st['msd_slow_tiles'] > 0, (k, wide)
            if variant == 'partial_symbol' and wide:
                assert st['key_bits'] % st['code_bits'] != 0          # the switch took effect


@pytest.mark.parametrize('variant', list(LOCAL_VARIANTS))
def test_word_at_the_tail_of_the_text(oracle, monkeypatch, variant):
    """The last copy of the word ends 0, 1, 7, 8, 15, 16 bytes before the final newline, in texts whose length is no
    multiple of 16: key packing reads 32 bytes per thread and must see zeros past the end."""
    _env(monkeypatch, PSS_MSD=1, **LOCAL_VARIANTS[variant])
    for d in E.TAIL_DS:
        t, want = _case(oracle, ('tail', d), lambda: E.tail_case(d))
        st = _build(t, want, (d, variant))
        assert st['msd'] == 1 and st['msd_slow_tiles'] > 0            # (70 copies)


# ---- 4. rounds: group-size tiers -------------------------------------------------------------------------------------

TIER_VARIANTS = {
    'default': {}, 'no_mid_tier': {'PSS_NO_MID_TIER': '1'}, 'no_mid_merge': {'PSS_NO_MID_MERGE': '1'},
    'big_merge0': {'PSS_BIG_MERGE': '0'}, 'big_merge1': {'PSS_BIG_MERGE': '1'}, 'big_merge2': {'PSS_BIG_MERGE': '2'},
    'no_big_merge': {'PSS_BIG_MERGE': '1', 'PSS_NO_BIG_MERGE': '1'}, 'count_sort': {'PSS_COUNT_SORT': '1'},
    'anchor0': {'PSS_ANCHOR': '0'}, 'anchor1': {'PSS_ANCHOR': '1'},
    'dense': {'PSS_MODE': 'dense'}, 'sparse': {'PSS_MODE': 'sparse'}, 'text': {'PSS_MODE': 'text'},
}
_STAT_KEYS = ('rounds', 'text_rounds', 'round_passes', 'sum_active', 'sort_elems', 'big_elems', 'mode', 'initial_passes')


def _stays_big(variant, shape, k):
    """Does a text of tier_case(k, shape) leave members to the chained sorts / the segmented merge (see the test below)?"""
    if variant == 'no_mid_tier':
        return k > E.GS_CAP
    if variant == 'no_mid_merge' and E.GS_CAP < k <= E.MID_CAP:
        return {'plain': 0, 'second': k // 2, 'crowded': k - 3}[shape] > E.MID_KMAX
    return k > E.MID_CAP


@pytest.mark.parametrize('variant', list(TIER_VARIANTS))
def test_groups_of_exactly_k_in_every_tier(oracle, monkeypatch, variant):
    """Groups of exactly k tied suffixes at every position of the planted word, k on both sides of GS_CAP = 512 (ranked in
    LDS up to it), MID_CAP = 4096 (one workgroup per group up to it) and two BG_TILE = 4096 tiles of the segmented merge --
    plain, with half of every group sharing a second word (one sub-group of k / 2 and k / 2 singletons, partial tiles), and
    with all but three members going on with the same 5 bytes (k - 3 equal keys in one bin: MID_KMAX = 512).
    big_elems counts the members that stayed with the chained sorts or the segmented merge: the largest group is exactly
    k, so it is zero up to the tier's limit and positive beyond -- 4096 by default, 512 without the middle tier.  Without
    the middle tier's merge sort (PSS_NO_MID_MERGE) a group of 513 .. 4096 stays behind when more than MID_KMAX = 512 of its
    keys share a bin: k // 2 of them with the second word, k - 3 with the common run (a group whose keys are ALL equal is
    in order as it stands and leaves the tier at once).  How many rounds see the groups depends on the mode: the sum is
    the one the CPU model of the rounds walks (tests/rounds_model.py: rounds, text_rounds, sum_active, big_elems and mode,
    for equality), under every variant but the forced anchor round, which the model leaves out -- from the key the build
    chose, wherever no round used periodic keys, the other part the model leaves out.  PSS_NO_BIG_MERGE=1 on top of
    PSS_BIG_MERGE=1 must walk exactly as PSS_BIG_MERGE=0 does."""
    _env(monkeypatch, **TIER_VARIANTS[variant])
    walked = 0
    for shape in ('plain', 'second', 'crowded'):
        for k in E.TIER_KS:
            t, want = _case(oracle, ('tier', k, shape), lambda: E.tier_case(k, shape))
            st = _build(t, want, (k, shape, variant))
            stats = tuple(st[s] for s in _STAT_KEYS)
            if variant != 'sparse':
                assert (st['big_elems'] > 0) == _stays_big(variant, shape, k), (k, shape, variant, st['big_elems'])
            if variant != 'anchor1' and st['periodic_rounds'] == 0:
                assert st['msd'] == st['ss'] == st['anchor'] == 0, (k, shape, variant)
                params = {x: int(st[x]) for x in ('key_chars', 'key_bits', 'code_bits')}
                w = M.tier_walk(k, shape, TIER_VARIANTS[variant], t, params)
                walked += 1
                got = tuple(int(st[x]) for x in M.TOTALS)
                assert got == w.totals(), '%s: the build reports %s = %s, the model walks\n%s' % ((k, shape, variant), M.TOTALS, got, w)
            if variant == 'no_big_merge':
                monkeypatch.delenv('PSS_NO_BIG_MERGE')
                monkeypatch.setenv('PSS_BIG_MERGE', '0')
                st0 = _build(t, want, (k, shape, 'big_merge0'))
                _env(monkeypatch, **TIER_VARIANTS[variant])
                assert tuple(st0[s] for s in _STAT_KEYS) == stats, (k, shape)
    print(variant, 'walks compared', walked)
    assert variant == 'anchor1' or walked > 0


@pytest.mark.parametrize('merge', [True, False])
def test_crowded_bin_of_the_middle_tier(oracle, monkeypatch, merge):
    """MID_KMAX = 512 on both sides: groups of 515 and 516 whose members all go on alike but three -- a bin of 512, which
    the counting kernel ranks, and of 513, which it hands to the merge sort (default: nothing reaches the chained sorts) or
    leaves flagged for the chained sorts (PSS_NO_MID_MERGE=1: big_elems > 0)."""
    if not merge:
        _env(monkeypatch, PSS_NO_MID_MERGE=1)
    for k in (E.MID_KMAX + 3, E.MID_KMAX + 4):
        t, want = _case(oracle, ('tier', k, 'crowded'), lambda: E.tier_case(k, 'crowded'))
        st = _build(t, want, (k, merge))
        assert (st['big_elems'] > 0) == (not merge and k - 3 > E.MID_KMAX), (k, merge, st['big_elems'])


# ---- 5. the remaining switches ---------------------------------------------------------------------------------------

def _switch_texts(oracle):
    out = []
    for kind, n in ((0, 1 << 19), (1, 1 << 19), (5, 1 << 20), (6, 1 << 20), (7, 1 << 20)):
        out.append(_case(oracle, ('corpus', kind), lambda: gen_corpus(kind, n)))
    out.append(_case(oracle, ('planted600',), E.switch_planted))
    return out


def _builds(oracle, note):
    """One build of every text with the environment as it stands: the statistics, suffix arrays compared."""
    out = []
    for i, (t, want) in enumerate(_switch_texts(oracle)):
        st = {}
        sa = sa_device(np.asarray(t), st)
        assert np.array_equal(sa, want), (note, i)
        st['n'] = t.size
        out.append(st)
    return out


def test_no_ties_pass(oracle, monkeypatch):
    """PSS_NO_TIES_PASS=1: plain key passes, no tie flags -- and without flags neither the MSD sort nor the sample sort is
    ever tried, even when forced."""
    _env(monkeypatch, PSS_MSD=1)
    assert any(st['msd'] == 1 for st in _builds(oracle, 'msd'))
    _env(monkeypatch, PSS_NO_TIES_PASS=1)
    for st in _builds(oracle, 'no ties pass'):
        assert (st['msd'], st['msd_buckets'], st['ss']) == (0, 0, 0)


@pytest.mark.parametrize('kind', [0, 1])
def test_no_sample_at_2p24(oracle, monkeypatch, kind):
    """PSS_NO_SAMPLE=1 at n = 2^24 (below, no build draws the sizing sample): the key is sized from the symbol counts.
    `lines` then never reaches the MSD sort, which is only taken on the sample's word (the default takes it:
    test_msd_is_chosen_for_high_entropy_text_only); `words` takes the sample sort either way -- it asks for the size of
    the text only -- so there the suffix array is all there is to compare."""
    _env(monkeypatch, PSS_NO_SAMPLE=1)
    t = gen_corpus(kind, 1 << 24)
    st = {}
    sa = sa_device(t, st, flags=8)
    assert hashlib.sha256(sa.tobytes()).hexdigest() == hashlib.sha256(oracle.sa(t).tobytes()).hexdigest()
    assert st['plan_hint'] == 0
    if kind == 0:
        assert (st['msd'], st['msd_buckets']) == (0, 0)
    else:
        assert st['ss'] == 1


@pytest.mark.parametrize('cap', [24, 33, 40])
def test_msd_key_cap(oracle, monkeypatch, cap):
    """PSS_MSD_KEY_CAP: the MSD sort's key is the whole symbols that fit the cap (the rounds do the rest)."""
    _env(monkeypatch, PSS_MSD=1, PSS_MSD_KEY_CAP=cap)
    took = 0
    for st in _builds(oracle, cap):
        if st['msd']:
            took += 1
            assert st['key_bits'] == (cap // st['code_bits']) * st['code_bits'] and st['key_bits'] >= 21
    assert took >= 2


def _probe_base(monkeypatch):
    # the probe runs before the first text round when the anchor round could follow at once: anchors on at any size, and
    # a narrowest window that the initial key's depth already covers (h >= window + 3)
    _env(monkeypatch, PSS_ANCHOR=1, PSS_ANCHOR_MIN_OMEGA=3)


def test_no_probe(oracle, monkeypatch):
    """PSS_NO_PROBE=1: the ties are not sampled (probe_pairs stays 0) and a text round always comes first."""
    _probe_base(monkeypatch)
    assert any(st['probe_pairs'] > 0 for st in _builds(oracle, 'probe'))
    _env(monkeypatch, PSS_NO_PROBE=1)
    for st in _builds(oracle, 'no probe'):
        assert st['probe_pairs'] == 0 and st['anchor_left'] == 0


@pytest.mark.parametrize('pct', [0, 90])
def test_probe_skip_pct(oracle, monkeypatch, pct):
    """PSS_PROBE_SKIP_PCT: no text round at all when more than this share of the sampled tied pairs go on alike."""
    _probe_base(monkeypatch)
    _env(monkeypatch, PSS_PROBE_SKIP_PCT=pct)
    probed = hit = 0
    for st in _builds(oracle, pct):
        assert st['anchor_left'] == 0
        if st['probe_pairs'] >= 64:
            probed += 1
            skipped = st['probe_same'] * 100 > st['probe_pairs'] * pct
            print(pct, st['probe_pairs'], st['probe_same'], st['text_rounds'])
            if skipped:           # (not skipped: the text round may still give up at once, large groups)
                hit += 1
                assert st['text_rounds'] == 0, (pct, st['probe_pairs'], st['probe_same'], st['text_rounds'])
    assert probed >= 1 and (pct != 0 or hit >= 1)      # (the planted text at least: its tied pairs go on alike for 48 symbols)


@pytest.mark.parametrize('omega', [3, 7, 9])
def test_anchor_min_omega(oracle, monkeypatch, omega):
    """PSS_ANCHOR_MIN_OMEGA: with the anchor round forced the narrowest window only decides whether the ties are sampled
    before the first text round -- when the initial key is omega + 3 symbols deep."""
    _env(monkeypatch, PSS_ANCHOR=1, PSS_ANCHOR_MIN_OMEGA=omega)
    sts = _builds(oracle, omega)
    for st in sts:
        h0 = st['key_chars'] - (1 if st['key_bits'] < st['key_chars'] * st['code_bits'] else 0)
        assert st['anchor_left'] == 0
        if st['probe_pairs'] > 0:
            assert h0 >= omega + 3
    if omega == 3:
        assert any(st['probe_pairs'] > 0 for st in sts)


@pytest.mark.parametrize('div', [3, 4])
def test_anchor_cap_div(oracle, monkeypatch, div):
    """PSS_ANCHOR_CAP_DIV with the window capped at 9: the round runs exactly when the windows chose at most n / div
    anchors -- asserted for every build that counted anchors.  Whether `anchor` flips between 3 and 4 on one text is not
    claimed: minimizers of window w choose about 2 n / (w + 1) positions, n / 5 at w = 9 (below both limits: no flip), and
    about n / 4 where the depth reached allows only a window of 7 -- on the limit itself, either way round."""
    _env(monkeypatch, PSS_ANCHOR=1, PSS_ANCHOR_OMEGA=9, PSS_ANCHOR_CAP_DIV=div)
    tried = 0
    for st in _builds(oracle, div):
        assert st['anchor_left'] == 0
        if st['anchor_count'] > 0:
            tried += 1
            assert st['anchor'] == (1 if st['anchor_count'] <= st['n'] // div else 0), (st['anchor_count'], st['n'])
    assert tried >= 1
