"""CPU self-checks of the edge-case texts (tests/sa_edge_texts.py): every generator, for every size the GPU tests of
tests/test_sa_edges_gpu.py use, must pass the checks built into it -- the planted word and its lead occur exactly k
times, exactly k suffixes share the rest of the word, the modelled joint buckets have exactly the sizes the case is
about -- before any kernel sees the text."""
import numpy as np
import pytest

from tests import sa_edge_texts as E


@pytest.mark.parametrize('k', E.BUCKET_KS)
def test_bucket_cases(k):
    t = E.bucket_case(k)
    assert (1 << 17) <= t.size <= (1 << 20) and int(E.bucket_sizes(t)[1].max()) == k


def test_tile_cases():
    counts = {}
    for name in ('pair8176', 'trio8177', 'run', 'chain'):
        t = E.tile_case(name)
        assert (1 << 17) <= t.size <= (1 << 20)
        counts[name] = [E.tile_count(t, lsd) for lsd in (True, False)]
    # one tile against a split, and nothing else differs between the two plans
    assert [b - a for a, b in zip(counts['pair8176'], counts['trio8177'])] == [1, 1]
    numbers, sizes = E.bucket_sizes(E.tile_case('run'))
    heads = E.tile_heads(numbers, sizes, int(sizes.sum()), True)
    assert heads[-4:].tolist() == [True, False, False, True]          # the window's last bucket goes alone
    numbers, sizes = E.bucket_sizes(E.tile_case('chain'))
    # 4088 after 4088 after 4088 from slot 3000 of a window: the first alone, the other two start inside the next window and fill
    # one tile to the last slot
    assert E.tile_heads(numbers, sizes, int(sizes.sum()), True)[-3:].tolist() == [True, True, False]


@pytest.mark.parametrize('lsd', [True, False])
def test_tagblock_cases(lsd):
    span = E.MSD_RAW_TAG_SPAN if lsd else E.MSD_TAG_SPAN
    for big in (False, True):
        t = E.tagblock_case(big, lsd)
        numbers, sizes = E.bucket_sizes(t)
        heads = E.tile_heads(numbers, sizes, t.size, lsd)
        # more buckets in a row than a tag block holds: without the block rule a window's worth would share a tile
        per_window = np.bincount(np.cumsum(sizes)[:-1] // E.MSD_WIN)
        assert per_window.max() > span and heads.sum() >= len(sizes) // span
        if big:
            at = len(sizes) - 1
            assert sizes[at] == 3000 and (E.lsd_numbers(numbers)[at] if lsd else at) % span == 0 and heads[at]


def test_bin_tail_tier_and_switch_cases():
    for k in E.BIN_KS:
        for wide in (False, True):
            assert E.bin_case(k, wide).size % 16
    for d in E.TAIL_DS:
        assert E.tail_case(d).size % 16
    for k in E.TIER_KS:
        for variant in ('plain', 'second', 'crowded'):
            assert E.tier_case(k, variant).size <= (1 << 20)
    for k in (E.MID_KMAX + 3, E.MID_KMAX + 4):
        assert E.tier_case(k, 'crowded').size <= (1 << 20)
    assert E.switch_planted().size <= (1 << 20)


def test_bucket_model_by_hand():
    """b'ba\\n': codes a = 2, b = 3, newline = 1 in 2 bits; ten symbols cover 20 bits."""
    got = E.joint_buckets(np.frombuffer(b'ba\n', dtype=np.uint8))
    assert got.tolist() == [(3 << 18) | (2 << 16) | (1 << 14), (2 << 18) | (1 << 16), 1 << 18]
    t = np.frombuffer(b'abcabd\n', dtype=np.uint8)
    assert E.joint_buckets(t, 3, 7, 21).tolist() == E.joint_buckets(t).tolist()
