"""The model of the rounds (tests/rounds_model.py) held to something that is not the model, on the CPU: its classes to a
sort of the zero-padded prefixes themselves, its last depth to a Kasai LCP of the oracle's suffix array, its totals to
its own list of rounds, and every pair of cases that stands on the two sides of one decision to walks the GPU test
(tests/test_rounds_gpu.py) can tell apart.  Every generator runs here (a generator asserts where its text sits)."""
import numpy as np
import pytest

from tests import rle_texts as R
from tests import rounds_model as M
from tests import sa_edge_texts as E

MODES = ({}, {'PSS_MODE': 'dense'}, {'PSS_MODE': 'text'}, {'PSS_MODE': 'sparse'}, {'PSS_MODE': 'text', 'PSS_TEXT_ROUNDS': '2'})


def _cut(t):
    """The first 2^12 - 1 bytes and a final newline."""
    return np.append(np.asarray(t[:M.SMALL - 1]), np.uint8(E.NL))


def _check_classes(t, key_chars, switches, note):
    w = M.walk(t, switches=switches, keep_classes=True, **M.params_of(t, key_chars))
    assert len(w.classes) == len([r for r in w.rounds_list if not r.gave_up]) + 1
    assert w.classes[0][0] == key_chars
    for depth, rank in w.classes:
        want = M.brute_ranks(t, depth)
        assert np.array_equal(rank, want), (note, switches, depth, str(w))
    # the list of every round is the suffixes that shared the round's depth with another one
    done = [r for r in w.rounds_list if not r.gave_up]
    for r, (depth, rank) in zip(done, w.classes):
        assert r.h == depth
        sizes = np.bincount(M.brute_ranks(t, depth))
        assert r.m == int(sizes[sizes > 1].sum()), (note, switches, r)
        if r.kind != 'global':
            limit = E.GS_CAP if 'PSS_NO_MID_TIER' in switches else E.MID_CAP
            assert r.nbig >= int(sizes[sizes > limit].sum())
            if 'PSS_NO_MID_MERGE' not in switches:
                assert r.nbig == int(sizes[sizes > limit].sum())
    return w


@pytest.mark.parametrize('name', list(M.CASES))
def test_classes_match_a_sort_of_the_prefixes(name):
    """The rank of every suffix at every depth the walk visits (1 + the suffixes with a smaller prefix of that many
    symbols, zeros past the end) against Python's sort of the prefixes: on the case's text cut to 2^12 bytes, under
    the case's switches and under every mode, and on the case's own families planted in 2^12 bytes where they fit."""
    case = M.CASES[name]
    t = _cut(case.text())
    for sw in (case.switches,) + MODES:
        _check_classes(t, case.key_chars, sw, name)
    if case.small is not None:
        small = case.small()
        assert small.size <= M.SMALL + 16
        w = _check_classes(small, case.key_chars, case.switches, name + ' small')
        # the planted families walk as they do in the full text: same kinds, same depths (the lists differ by the ties of
        # the random text itself, which 2^12 bytes over two symbols have and 2^16 over 39 have not)
        full = case.walk()
        if 'binary' not in name and 'mode' not in name:
            assert [r[:3] for r in w.rounds_list] == [r[:3] for r in full.rounds_list], (str(w), str(full))


def test_classes_of_tier_texts_and_large_groups():
    """2^12 bytes hold no planted group beyond a tier, so the members of the large groups are checked where they can be:
    E.tier_case cut short (small groups only: none) and one symbol repeated 1500 and 4200 times (one group of nearly everything at
    every depth: beyond GS_CAP, beyond MID_CAP, and global rounds)."""
    t = _cut(E.tier_case(511, 'second'))
    for sw in MODES + ({'PSS_NO_MID_TIER': '1'}, {'PSS_NO_MID_MERGE': '1'}):
        w = _check_classes(t, M.TIER_KEY_CHARS, sw, 'tier')
        assert w.big_elems == 0
    for count, sws in ((1500, ({'PSS_MODE': 'dense', 'PSS_NO_MID_TIER': '1'}, {'PSS_NO_MID_TIER': '1'})), (4200, ({'PSS_MODE': 'dense'}, {}))):
        run = np.append(np.full(count, 97, np.uint8), np.uint8(E.NL))
        for sw in sws:
            w = _check_classes(run, 4, sw, 'run')
            assert w.big_elems > 0 and 'global' in [r.kind for r in w.rounds_list], str(w)


def test_crowded_bins_of_the_middle_tier():
    """_crowded on groups written by hand: 600 members of which 513 | 512 carry one key, all keys equal, keys that differ
    in bit 40 only (bins on bits 29 .. 40: two bins of 300), and a group of 512 (not the middle tier's)."""
    def full(count, value):
        return np.full(count, value, np.uint64)

    def one(*parts):
        keys = np.concatenate([np.asarray(p, np.uint64) for p in parts])
        n = keys.size
        rank, size, act = np.full(n, 7, np.int64), np.full(n, n, np.int64), np.arange(n)
        return M._crowded(rank, size, act, keys)
    spread = np.arange(6, 93, dtype=np.uint64) << np.uint64(20)            # (87 other keys, one per bin)
    assert one(full(513, 5 << 20), spread) == 600
    assert one(full(512, 5 << 20), spread, [99 << 20]) == 0
    assert one(full(600, 9)) == 0
    assert one(full(300, 1 << 40), full(300, 0)) == 0
    assert one(full(520, (1 << 40) + 3), full(80, 0)) == 600          # (3 is below the binned bits)
    assert one(full(500, 1), full(12, 0)) == 0                       # 512 members: ranked in LDS before
    # two groups in one list: only the crowded one counts
    keys = np.concatenate([full(513, 5 << 20), spread, np.arange(700, dtype=np.uint64)])
    rank = np.concatenate([np.full(600, 1), np.full(700, 601)]).astype(np.int64)
    size = np.concatenate([np.full(600, 600), np.full(700, 700)]).astype(np.int64)
    assert M._crowded(rank, size, np.arange(1300), keys) == 600


@pytest.mark.parametrize('name', list(M.CASES))
def test_final_depth_against_the_lcp(oracle, name):
    """Nothing is tied at the depth the walk ends with, and something was at the depth its last round started from: the
    largest LCP of neighbours in the oracle's suffix array lies between them."""
    case = M.CASES[name]
    t = case.text()
    w = case.walk()
    top = max(M.kasai(t, oracle.sa(np.asarray(t))))
    assert w.h_final >= top + 1, (w.h_final, top)
    if w.rounds_list:
        assert w.rounds_list[-1].h <= top, (str(w), top)
    else:
        assert top < w.h0


def test_the_two_sides_of_every_edge_walk_differently():
    """A pair of cases that differ in neither rounds, text_rounds, sum_active, big_elems nor mode is no pair: a build could
    take either side and report the same."""
    assert len(M.EDGES) >= 40 and {x for e in M.EDGES for x in e} <= set(M.CASES)
    for a, b in M.EDGES:
        wa, wb = M.CASES[a].walk(), M.CASES[b].walk()
        assert wa.totals() != wb.totals(), (a, b, str(wa), str(wb))
    # every case belongs to an edge, except the two that show one behaviour
    assert set(M.CASES) - {x for e in M.EDGES for x in e} == {'global_then_local', 'dominating'}


@pytest.mark.parametrize('name', list(M.CASES))
def test_totals_follow_from_the_rounds(name):
    w = M.CASES[name].walk()
    rounds = text_rounds = sum_active = big_elems = 0
    for r in w.rounds_list:
        assert r.kind in ('text', 'rank', 'global') and r.m >= 2 and 0 <= r.nbig <= r.m
        assert not r.gave_up or r.kind == 'text'
        if r.gave_up:
            continue
        rounds += 1
        text_rounds += r.kind == 'text'
        sum_active += r.m
        big_elems += 0 if r.kind == 'global' else r.nbig
    assert (rounds, text_rounds, sum_active, big_elems) == w.totals()[:4]
    kinds = [r.kind for r in w.rounds_list if not r.gave_up]
    assert kinds == sorted(kinds, key=lambda k: k != 'text')                   # text rounds come first
    if w.first_mode == M.M_SPARSE:
        assert set(kinds) <= {'global'} and w.mode == 1
    elif w.first_mode == M.M_TEXT:
        assert (w.mode == 2) == (w.rounds_list[-1].kind == 'text' and not w.rounds_list[-1].gave_up)
    else:
        assert w.mode == 0 and 'text' not in kinds
    # a list never grows, depths never shrink
    for p, q in zip(w.rounds_list, w.rounds_list[1:]):
        assert q.m <= p.m and q.h >= p.h


def test_reduced_string_of_the_run_length_path():
    """The rounds of the run-length path sort the string of run symbols, rank rounds from depth 1: 512 runs of 8 bytes,
    a and b in turn, walk in 9 rounds over 512 * 9 - (0 + 1 + 3 + ... + 255) = 4106 list members -- the figures
    tests/test_sa_gpu.py pins by hand -- and the reduced strings of R.tier_case match a sort of their prefixes."""
    t = np.frombuffer((b'a' * 8 + b'b' * 8) * 256, dtype=np.uint8)
    w = M.walk(R.model(t).meta, key_chars=1, key_bits=1, code_bits=1, switches={}, rank_only=True)
    assert (w.rounds, w.sum_active, w.mode, w.text_rounds) == (9, 4106, 0, 0)
    assert [r.m for r in w.rounds_list] == [512 - (h - 1) for h in (1, 2, 4, 8, 16, 32, 64, 128, 256)]
    meta = R.model(R.tier_case(513)).meta[:3000]
    w = M.walk(meta, key_chars=1, key_bits=1, code_bits=1, switches={}, rank_only=True, keep_classes=True)
    assert w.rounds >= 3
    for depth, rank in w.classes:
        assert np.array_equal(rank, M.brute_ranks(meta, depth)), depth


def test_rules_on_their_edges():
    """The restated rules of rounds_layout.h at the values the cases stand on."""
    assert M.first_mode(65536, 64, -1, 5, False) == M.M_SPARSE and M.first_mode(65536, 65, -1, 5, False) == M.M_TEXT
    assert M.first_mode(65536, 4096, 1, 5, False) == M.M_SPARSE and M.first_mode(65536, 4097, 1, 5, False) == M.M_TEXT
    assert M.first_mode(65536, 0, 2, 5, False) == M.M_SPARSE and M.first_mode(65536, 9, 2, 0, False) == M.M_DENSE
    assert M.first_mode(65536, 9, -1, 5, True) == M.M_DENSE
    assert not M.text_round_gives_up(3, 4, 0) and M.text_round_gives_up(4, 5, 0) and not M.text_round_gives_up(3, 5, 0)
    assert not M.text_round_gives_up(2, 4, 1) and M.text_round_gives_up(3, 5, 1)
    assert M.text_progress(6, 10, 1) and not M.text_progress(61, 100, 1) and M.text_progress(99, 1, 0)
    assert M.goes_global(0.5, False, 100) == 0 and M.goes_global(51 / 100, False, 101) == 50 and M.goes_global(0.9, True, 100) == 0
    assert [M.symbols_per_key(b) for b in (2, 3, 4, 6, 7, 8, 9)] == [16, 16, 16, 10, 9, 8, 7]
