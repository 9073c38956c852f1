"""tests/lsd_texts.py on the CPU: the model of the LSD radix sort against a plain brute force (tuples of symbols through
`sorted`), its pass-by-pass replay against its one-argsort answer at every prefix of a run, and every planted text that
tests/test_lsd_edges_gpu.py uses against the routes it is there to walk -- conditions on the inputs, asserted here so
that a later change of a generator cannot quietly drop a route."""
import numpy as np
import pytest

from tests import lsd_texts as L


def test_geometry():
    """The shipped cap keeps one tile per range up to 1024 tiles; a cap of 8 gives three tiles per range from 65537 on."""
    assert L.geometry(1) == (1, 1, 8) and L.geometry(4097) == (2, 1, 8) and L.geometry(8 * 4096 + 1) == (9, 1, 16)
    assert L.geometry(1024 * 4096) == (1024, 1, 1024)
    assert L.geometry((1 << 22) + 1) == (1025, 2, 520)             # 513 ranges in use, the last one holds one element
    assert L.geometry(8 * 4096, 8) == (8, 1, 8) and L.geometry(8 * 4096 + 1, 8) == (9, 2, 8)      # 5 in use, 3 empty
    assert L.geometry(65536, 8) == (16, 2, 8) and L.geometry(65537, 8) == (17, 3, 8)
    assert L.geometry(69631, 8) == (17, 3, 8) and 69631 % 4096 == 4095
    assert L.geometry(98304, 8) == (24, 3, 8) and L.geometry(98305, 8) == (25, 4, 8)
    assert L.geometry(3 * 8 * 4096, 8)[1] == 3 and L.geometry(3 * 8 * 4096 + 1, 8)[1] == 4


def _read_rank(i):
    """Where suffix i stands among equal keys: tile, wave, round r of its thread, lane (L.read_order, restated)."""
    return (i // 4096, (i % 4096) // 1024, i % 16, (i % 1024) // 16)


def test_read_order():
    for n in (1, 17, 4095, 4096, 4097, 9000):
        assert L.read_order(n).tolist() == sorted(range(n), key=_read_rank)


def _brute_keys(sym, b, k, drop):
    """Keys by Python integers from the symbols of the text (zero past the end)."""
    n = len(sym)
    ext = list(sym) + [0] * k
    out = []
    for i in range(n):
        v = 0
        for j in range(k):
            v = (v << b) | ext[i + j]
        out.append(v >> drop)
    return out


@pytest.mark.parametrize('cfg', L.CONFIGS)
def test_model_against_brute_force(cfg):
    """pack_keys, want_suffix (with and without flags, at every key width the case runs at) and want_pairs on tiny texts
    of few symbols -- many ties, many keys that reach past the end -- against Python integers and `sorted`."""
    b, k, drop, plus_one = cfg
    rng = np.random.default_rng(b * 100 + k)
    a = L.alphabet(b, plus_one)
    for n in (1, 2, 3, 17, 60):
        t = a[rng.integers(0, min(3, a.size), n)].astype(np.uint8)
        codes = L.padded(t, plus_one)
        keys = L.pack_keys(codes, n, b, k, plus_one, drop)
        brute = _brute_keys([int(c) + plus_one for c in t], b, k, drop)
        assert [int(x) for x in keys] == brute
        # the key orders as the tuple of its symbols does (drop only coarsens the last one)
        sym = [int(c) + plus_one for c in t] + [0] * k
        tup = [tuple(sym[i:i + k - 1]) + (sym[i + k - 1] >> drop,) for i in range(n)]
        assert sorted(range(n), key=lambda i: (tup[i], i)) == sorted(range(n), key=lambda i: (brute[i], i))
        for kb in L.sweep_of(cfg):
            m = (1 << (8 * ((kb + 7) // 8))) - 1
            order = sorted(range(n), key=lambda i: (brute[i] & m,) + _read_rank(i))
            want = [i | ((1 << 31) if j and (brute[i] & m) == (brute[order[j - 1]] & m) else 0) for j, i in enumerate(order)]
            assert L.want_suffix(keys, kb).tolist() == want
            assert L.want_suffix(keys, kb, flags=False).tolist() == order
            for mask in (0xffffffff, 0x3f, 0xfe, 0x02):
                dm = sum(0xff << (8 * p) for p in range((kb + 7) // 8) if (mask >> p) & 1)
                o2 = sorted(range(n), key=lambda i: (brute[i] & dm, i))
                wk, wv = L.want_pairs(keys, np.arange(n, dtype=np.uint32), kb, mask)
                assert wv.tolist() == o2 and [int(x) for x in wk] == [brute[i] for i in o2]


def _check_replay(keys, width, cap):
    """Every pass of the replay -- flags from group numbers, route by route -- equals the one-argsort answer for that prefix."""
    passes = L.replay(keys, width, cap)
    for p, (out, _, _) in enumerate(passes):
        kb = min(8 * (p + 1), width)
        assert np.array_equal(out, L.want_suffix(keys, kb)), (p, kb)
    return passes


@pytest.mark.parametrize('cfg', L.CONFIGS)
def test_planted_texts_walk_every_route(cfg):
    """The census conditions of every planted text at cap 8: from pass 1 on, tied and untied elements on in_tile, carry and
    fix in EVERY pass, and on carry_skip and fix_skip in some pass; in pass 0 (everything tied) an element on each route."""
    b, k, drop, plus_one = cfg
    for n in L.PLANTED_NS:
        t = L.planted(cfg, n)
        assert t.dtype == np.uint8 and t.size == n and np.isin(t, L.alphabet(b, plus_one)).all()
        keys = L.pack_keys(L.padded(t, plus_one), n, b, k, plus_one, drop)
        width = L.key_width(cfg)
        _check_replay(keys, width, L.CAP)
        per_pass, empty, last = L.census(keys, width, L.CAP)
        assert L.census_ok(per_pass) == [], (cfg, n, per_pass)
        assert len(per_pass) == L.passes_of(width)
        tiles, tpr, ranges = L.geometry(n, L.CAP)
        assert tpr >= 3 and ranges == 8 and empty == 8 - (tiles + tpr - 1) // tpr and last == n - (tiles - 1) * L.RS_TILE


def test_census_on_a_text_worked_by_hand():
    """A census counted by hand: one symbol is one digit (8 bits, 2 symbols, a 16-bit key), nine tiles, two per range at
    cap 8, symbol 7 everywhere except a 9 in tiles 0, 1, 4 and at the very end -- in pass 0 the digit is the SECOND symbol
    of the key, so the suffix in front of each 9 carries it."""
    n = 8 * 4096 + 1
    assert L.geometry(n, 8) == (9, 2, 8)
    t = np.full(n, 7, dtype=np.uint8)
    t[[11, 4096 + 11, 4 * 4096 + 11, 8 * 4096]] = 9
    keys = L.pack_keys(L.padded(t, 0), n, 8, 2, 0, 0)
    per_pass, empty, last = L.census(keys, 16, 8)
    assert (empty, last) == (3, 1)
    # pass 0, digit 9 (suffixes 10, 4106, 16394, 32767 -- the one before each 9): tile 0 -> 1 is a carry, tile 1 (range 0) ->
    # tile 4 (range 2) skips range 1, tile 4 (range 2) -> tile 7 (range 3) is a plain fix; the last suffix (9 0) has digit 0
    # digit 7 is everywhere up to tile 7: it crosses the 4 tile borders inside ranges 0 .. 3 and the 3 borders between them
    # (the one element of range 4 has digit 0)
    assert per_pass[0]['carry'] == (0, 1 + 4) and per_pass[0]['fix_skip'] == (0, 1) and per_pass[0]['carry_skip'] == (0, 0)
    assert per_pass[0]['fix'] == (0, 1 + 3) and per_pass[0]['in_tile'][0] == 0
    assert sum(sum(v) for v in per_pass[0].values()) == n - 3                        # three digits, each with one first element
    _check_replay(keys, 16, 8)


def test_tail_cases():
    """The texts of the tail test: the planted word's copies are tied on the whole key, and the cut copy at the very end --
    whose key goes on past the end of the text -- sorts directly in front of them, untied unless nothing is cut."""
    for cfg in L.TAIL_CONFIGS:
        b, k, drop, plus_one = cfg
        for n in L.TAIL_NS:
            for reach in L.TAIL_REACH:
                if reach > k:
                    continue
                t, word = L.tail_case(n, cfg, reach)
                assert t.size == n
                keys = L.pack_keys(L.padded(t, plus_one), n, b, k, plus_one, drop)
                want = L.want_suffix(keys, L.key_width(cfg))
                wkey = int(L.pack_keys(L.padded(word, plus_one), k, b, k, plus_one, drop)[0])
                group = np.flatnonzero(keys[want & 0x7fffffff] == np.uint64(wkey))
                copies = L.TAIL_COPIES + (1 if reach == 0 else 0)
                assert group.size >= copies and (want[group[1:]] >> 31).all() and not (want[group[0]] >> 31)
                if 0 < reach < k:
                    cut = n - (k - reach)
                    # (below the word's key; with dropped bits a cut of one symbol may coarsen to the same key)
                    assert int(keys[cut]) <= wkey and (drop or int(keys[cut]) < wkey)
                _check_replay(keys, L.key_width(cfg), L.CAP)
