"""Search within k mismatches (Reader.search_near_ids_batch / search_near_batch_packed / count_near_bytes and the str
conveniences) against the brute-force reference of tests/near_ref.py.  Every pattern of every batch goes through one
check():
  * per pattern, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk by the first exact piece of each entry's leftmost near
    match, inside one piece by the suffix at that piece's occurrence (the reference sorts the suffixes themselves);
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result, and every entry's text is the
    reference's for its id;
  * `hits` is the sum of the pieces' exact occurrences (near_ref.piece_hits);
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), none of ANCHORED, MID, SMALL_*, RESIDENT,
    SA_ORDER.
The cases: exactly k mismatches against k + 1 with every piece in turn the only exact one; repeated and nested pieces;
windows across a newline and at the chunk's two ends; the leftward scan for an earlier window within budget (same word,
same 64-byte step, one and two steps back, overlapping, at every (lane, byte)); pattern lengths around the load widths
at every alignment; 0x00 and high bytes; mixed budgets; k = 0 against search_ids_batch; more candidates than the mid
pipeline holds; the three interval routes; placement; errors and conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, near_pieces
from tests import search_harness as H
from tests.near_ref import NearRef
from tests.search_harness import FILLER, R, device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu

WORD = b'qrstuvwxyz1234567890QRSTUVWXYZ'          # (no byte of the filler, no byte twice)


def subst(p, positions, by=b'#'):
    """p with the bytes at `positions` replaced by `by` (a byte p does not hold)."""
    a = bytearray(p)
    for i in positions:
        assert a[i] != by[0]
        a[i] = by[0]
    return bytes(a)


def check(r, ref, patterns, k, **kw):
    """patterns within k (one int, or one per pattern) on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.NEAR, r, ref, (list(patterns), k), **kw)


def one_chunk(lines, closed=True):
    return H.one_chunk(NearRef, lines, closed)


# ---- 1. what matches and what does not ----------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_exactly_k_mismatches_match_and_k_plus_one_do_not(k):
    """Per piece j in turn, entries in which piece j is the ONLY exact piece: one substitution in every other piece, moved
    through every position of those pieces -- k mismatches, a match.  Beside each, the same with one more substitution:
    inside piece j (no piece is exact: not even a candidate) and inside another piece (piece j is a candidate, and the
    count rejects it).  And the pattern itself, where every piece is exact: the entry comes once."""
    rng = np.random.default_rng(1520 + k)
    P = WORD[:11 + k]                                      # (pieces of unequal length for k > 0)
    cut = near_pieces(P, k)
    lines, good, bad = [], [], []
    for j in range(k + 1):
        others = [c for i, c in enumerate(cut) if i != j]
        for s in range(max(len(piece) for _, piece in cut)):
            at = [off + s % len(piece) for off, piece in others]
            assert len(at) == k
            for body, ok in [(subst(P, at), True), (subst(P, at + [cut[j][0] + s % len(cut[j][1])]), False)] + \
                            ([(subst(P, at + [others[0][0] + (s + 1) % len(others[0][1])]), False)] if k and len(others[0][1]) > 1 else []):
                (good if ok else bad).append(len(lines))
                lines.append(filler(rng, int(rng.integers(0, 20))) + body + filler(rng, int(rng.integers(0, 20))))
    for _ in range(3):
        good.append(len(lines))
        lines.append(filler(rng, int(rng.integers(0, 20))) + P + filler(rng, int(rng.integers(0, 20))))
    lines += [filler(rng, int(rng.integers(0, 40))) for _ in range(50)]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [P], k)
        assert sorted(res.ids.tolist()) == good and len(bad) >= (1 if k == 0 else 2 * k)
        if k:
            assert r.last_stats()['hits'] > r.last_stats()['entries']          # rejected candidates, and the exact entries' other pieces
    finally:
        r.close()


def test_repeated_and_nested_pieces_and_one_letter_entries():
    lines = [b'abab', b'abax', b'xbab', b'abxb', b'axab', b'xxab', b'abxx', b'ab', b'aba', b'ababab', b'xabab', b'ababx', b'bababa',
             b'aaaa', b'aaa', b'a', b'aaab', b'xxxa', b'axxx', b'xxxx', b'xaxx', b'aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa',
             b'aabaa', b'aabxa', b'xabaa', b'aaxaa', b'aab', b'baa', b'aaaab', b'aabaabaa', b'', b'b', b'bbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbb',
             b'abcabc', b'abcabd', b'abdabc', b'xbcabc', b'abcxbc']
    r, ref, data = one_chunk(lines)
    try:
        patterns = [(b'abab', 1), (b'aaaa', 3), (b'aaaa', 1), (b'aaaa', 0), (b'aabaa', 1), (b'aab', 1), (b'aaa', 2), (b'abcabc', 1), (b'abcabc', 2),
                    (b'a', 0), (b'ab', 1), (b'bbbb', 2), (b'bb', 1)]
        assert near_pieces(b'abab', 1) == [(0, b'ab'), (2, b'ab')] and near_pieces(b'aab', 1) == [(0, b'a'), (1, b'ab')]
        res = per_pattern(check(r, ref, [p for p, _ in patterns], [k for _, k in patterns]))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        assert {b'abab', b'abax', b'xbab', b'abxb', b'axab', b'ababab', b'xabab', b'ababx', b'bababa'} <= set(texts(res[0]))
        assert not {b'xxab', b'abxx', b'ab', b'aba', b'aaaa'} & set(texts(res[0]))
        # `aaaa` within 3: every entry of four bytes or more that holds an `a`
        assert texts(res[1]) == sorted(e for e in lines if any(b'a' in e[i:i + 4] for i in range(len(e) - 3)))
        assert b'a' * 73 in texts(res[1]) and b'b' * 32 in texts(res[11]) and b'b' * 32 in texts(res[12])
    finally:
        r.close()


# ---- 2. entry and chunk edges ------------------------------------------------------------------------------------------

def test_a_window_across_a_newline_is_no_match():
    """`..ab\\ncd..` holds abZcd within one mismatch only across the newline: no match, in either entry -- in the middle of
    the chunk, at its first entry and at its last, closed and unterminated.  The pieces `ab` and `Zcd` / `cd` hit all the
    same, so the candidates are there and are rejected by the entry bounds."""
    for closed in (True, False):
        lines = [b'ab', b'cd', b'xxab', b'cdxx', b'abZcd', b'abQcd', b'xab', b'cd', b'', b'ab', b'', b'cd', b'abcd', b'yyyyab', b'cd']
        r, ref, data = one_chunk(lines, closed)
        try:
            assert data.startswith(b'ab\ncd') and (data.endswith(b'ab\ncd\n') if closed else data.endswith(b'ab\ncd'))
            res = per_pattern(check(r, ref, [b'abZcd', b'abcd', b'abZcd', b'bZc', b'ab\ncd', b'b\nc'], [1, 1, 2, 1, 1, 1]))
            assert sorted(r.entries_by_id(res[0])) == [b'abQcd', b'abZcd'] and r.entries_by_id(res[1]) == [b'abcd']
            assert res[4].size == 0 and res[5].size == 0
            assert r.last_stats()['hits'] > 20
        finally:
            r.close()


def test_windows_that_would_leave_the_chunk():
    """A piece hit with di < off_j (the window would start before the text) and one with m + L > n (it would end past the
    text, on an unterminated chunk): rejected before anything is read.  Matches flush with the chunk's and the entries'
    two ends are kept."""
    P = b'qrstuvwx'
    texts = [b'uvwx opens\nqrstuvw',                     # `uvwx` at 0: m = -4; `qrst` at n - 7: the window ends one past n
             b'qrstuvwx',                                # the whole chunk is the pattern
             b'qrstuvw',                                 # one byte short
             b'q#stuvwx\nxx\nqrstuv#x',                  # flush with the chunk's start and end, one mismatch each
             b'uvwx',                                    # the whole chunk is the second piece
             b'#rstuvwx\n#rstuvw#\nqrstuvw#']
    r, ref = device_reader(texts), NearRef(texts)
    try:
        res = per_pattern(check(r, ref, [P, P, P], [0, 1, 2]))
        assert res[0].tolist() == [1 << 32]
        assert sorted(res[1].tolist()) == [1 << 32, 3 << 32, (3 << 32) | 2, 5 << 32, (5 << 32) | 2]
        assert sorted(res[2].tolist()) == [1 << 32, 3 << 32, (3 << 32) | 2, 5 << 32, (5 << 32) | 1, (5 << 32) | 2]
        # 0x00 as a pattern's last byte next to the chunk's end: the zero padding behind n is not text
        texts0 = [b'ab\x00', b'ab', b'xab\nab\x00\x00', b'a\x00\x00']
        r0, ref0 = device_reader(texts0), NearRef(texts0)
        try:
            res = per_pattern(check(r0, ref0, [b'ab\x00', b'ab\x00', b'ab\x00\x00', b'b\x00\x00\x00', b'\x00\x00'], [0, 1, 1, 1, 1]))
            assert res[0].tolist() == [0, (2 << 32) | 1] and res[2].tolist() == [(2 << 32) | 1]
            assert sorted(res[1].tolist()) == [0, (2 << 32) | 1, 3 << 32] and res[3].size == 0
        finally:
            r0.close()
    finally:
        r.close()


def test_matches_flush_with_the_entry_ends():
    rng = np.random.default_rng(1530)
    P = WORD[:13]
    lines = []
    for body in (P, subst(P, [0]), subst(P, [12]), subst(P, [0, 12]), subst(P, [5, 6])):
        lines += [body, body + filler(rng, 9), filler(rng, 9) + body, filler(rng, 70) + body, body + filler(rng, 70), b'']
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [P, P, P], [0, 1, 2])
        assert res.counts.tolist() == [5, 15, 25]
    finally:
        r.close()
    r, ref, data = one_chunk(lines[:-1], closed=False)      # the last entry, `P with two substitutions + filler`, is unterminated
    try:
        assert check(r, ref, [P, P, P], [0, 1, 2]).counts.tolist() == [5, 15, 25]
    finally:
        r.close()


# ---- 3. the leftward scan: an earlier window within budget ---------------------------------------------------------------

SCAN_PATTERNS = ((b'qr7', 1), (b'qrstuvwxyz12', 1), (b'qrstuvwxyz12', 3), (b'qrstuvwx', 2), (b'q7', 0))
GEOMS = {'word': (0, 4), 'word7': (1, 7), 'next_word': (7, 8), 'step': (3, 40), 'one_step_back': (3, 70), 'two_steps_back': (3, 140),
         'far': (60, 700), 'overlap': (2, 5)}


def test_an_earlier_window_within_budget_drops_the_hit():
    """The pattern twice in an entry: an exact occurrence to the RIGHT and, to its left, a window with exactly k
    substitutions (kept as the entry's match: the entry comes once) or with k + 1 (no match: the exact one stands).
    `overlap`: the two windows share bytes.  Every geometry with the entry shifted by 0 .. 3 bytes against the 8-byte
    grid of the text."""
    rng = np.random.default_rng(1531)
    lines = []
    for P, k in SCAN_PATTERNS:
        cut = near_pieces(P, k)
        within = subst(P, [off for off, _ in cut[1:]])                      # k substitutions: the first piece is exact
        beyond = subst(P, [off + len(piece) - 1 for off, piece in cut])       # k + 1: one in every piece
        for name, (a1, a2) in GEOMS.items():
            for lead in range(4):
                for first in (within, beyond, subst(P, [0]) if k else P):
                    e = bytearray(filler(rng, a2 + len(P) + int(rng.integers(0, 12))))
                    e[a1:a1 + len(P)] = first                   # (where the two overlap, the exact one is written over the earlier one's tail)
                    e[a2:a2 + len(P)] = P
                    lines += [b'#' * lead, bytes(e)]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [p for p, _ in SCAN_PATTERNS], [k for _, k in SCAN_PATTERNS])
        assert (res.counts >= 4 * 3 * len(GEOMS)).all()
        assert r.last_stats()['hits'] > 2 * r.last_stats()['entries']
    finally:
        r.close()


def test_every_lane_and_byte_of_the_first_step():
    """An earlier window within budget at every position 0 .. 65 in front of an exact occurrence at 80: the hit at 80 is
    dropped wherever the earlier one stands (the entry still comes once, for the earlier window); a window one mismatch
    over budget at the same positions changes nothing."""
    rng = np.random.default_rng(1532)
    lines = []
    for at in range(0, 66):
        for first in (b'qr#tu', b'#rstu', b'q#s#u', b'#rst#'):
            e = bytearray(filler(rng, 90))
            e[at:at + 5], e[80:85] = first, b'qrstu'
            lines.append(bytes(e))
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [b'qrstu', b'qrstu'], [1, 2])
        assert res.counts.tolist() == [264, 264]
        # (within 1 the entries of `qr#tu` and `#rstu` are kept at the earlier window, through its exact piece `qr` or `stu`:
        # piece 0's hits come first, so the order check above has seen both pieces lead)
        first = per_pattern(res)[0][:66].tolist()
        assert sorted(first) == [4 * at for at in range(66)]
    finally:
        r.close()


def test_an_earlier_window_in_the_same_word_and_a_mismatch_before_an_exact_match():
    lines = [b'pas5word password', b'password pas5word', b'xpassw0rdpassword', b'pa55word password', b'p@55word passw0rd x',
             b'passwordpassword', b'pasSworDpassword', b'ssword password', b'passwor', b'password', b'assword', b'p4ssw0rd']
    r, ref, data = one_chunk(lines)
    try:
        res = per_pattern(check(r, ref, [b'password'] * 4, [0, 1, 2, 3]))
        assert [x.size for x in res] == [8, 9, 10, 10]          # (`passwor` and `assword` are a byte short: a deletion, not a substitution)
    finally:
        r.close()


# ---- 4. load widths ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_pattern_lengths_around_the_load_widths_at_every_alignment(k):
    """Pattern lengths k + 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, each planted at every alignment m mod 8 with exactly k
    substitutions (a match) and with k + 1 (none), the last byte of the pattern among the substituted ones."""
    rng = np.random.default_rng(1540 + k)
    lengths = sorted({k + 1, 7, 8, 9, 15, 16, 17, 23, 24, 25})
    lines, patterns, want = [], [], []

    def add(body, lead):            # body in an entry of its own, at an offset of the chunk that is lead mod 8
        at = sum(len(x) + 1 for x in lines)
        lines.append(b'#' * ((lead - at) % 8) + body)

    for L in lengths:
        P = WORD[:L]
        cut = near_pieces(P, k)
        within = subst(P, [off + len(piece) - 1 for off, piece in cut[1:]])       # (the last byte among them when k > 0)
        beyond = subst(within, [cut[0][0] + len(cut[0][1]) - 1])
        patterns.append(P)
        want.append(0)
        for lead in range(8):
            add(within + filler(rng, int(rng.integers(0, 6))), lead)
            add(beyond, lead)
            want[-1] += 1
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, patterns, k)
        for P, c, w in zip(patterns, res.counts.tolist(), want):
            assert c >= w, (P, c, w)              # (a longer WORD prefix's entries hold the shorter ones within budget)
        assert res.counts.tolist()[-1] == 8
    finally:
        r.close()


# ---- 5. bytes, budgets and k = 0 -----------------------------------------------------------------------------------------

def test_zero_and_high_bytes_are_bytes_like_any_other():
    rng = np.random.default_rng(1550)
    abc = np.frombuffer(b'\x00\x80\xff\xc3\xa9\x7f\x01', np.uint8)
    lines = [bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 24)))]) for _ in range(300)]
    lines += [b'\x00' * 9, b'\xff' * 9, b'\x00\x00\x00', b'caf\xc3\xa9', b'caf\xc3\xa8', b'cafe']
    r, ref, data = one_chunk(lines, closed=False)
    try:
        patterns = [b'\x00\x00', b'\x00\x80\xff', b'\xff\xff\xff\xff', b'\xc3\xa9', b'caf\xc3\xa9', b'\x00' * 9, b'\x80\x00\x80\x00\x80', b'\x7f\x01\x00\x00']
        for k in (0, 1, 2):
            check(r, ref, [p for p in patterns if len(p) > k], k)
        res = per_pattern(check(r, ref, [b'caf\xc3\xa9', b'caf\xc3\xa9'], [0, 1]))
        assert r.entries_by_id(res[0]) == [b'caf\xc3\xa9'] and sorted(r.entries_by_id(res[1])) == [b'caf\xc3\xa8', b'caf\xc3\xa9']
    finally:
        r.close()


def test_mixed_budgets_and_k_zero_is_the_plain_search():
    rng = np.random.default_rng(1551)
    lines = [filler(rng, int(rng.integers(0, 30))) for _ in range(500)]
    r, ref, data = one_chunk(lines)
    try:
        patterns = [b'a', b'ab', b'abc', b'mnop', b'pon', b'zz', b'abcdefgh', b'ponmlk', b'p', b'hgf']
        patterns += [lines[int(i)][1:int(rng.integers(3, 12))] for i in rng.integers(0, len(lines), 30) if len(lines[int(i)]) >= 12]
        got, plain = check(r, ref, patterns, 0), r.search_ids_batch(patterns)
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts) and got.ids.size > 500
        ks = [min(int(rng.integers(0, 4)), len(p) - 1) for p in patterns]
        assert {0, 1, 2, 3} <= set(ks)
        mixed = check(r, ref, patterns, ks)
        for k in range(4):          # every pattern of the mixed batch: what a batch of its own budget returns
            some = [i for i, kk in enumerate(ks) if kk == k]
            alone = per_pattern(check(r, ref, [patterns[i] for i in some], k))
            for i, ids in zip(some, alone):
                assert np.array_equal(per_pattern(mixed)[i], ids), (patterns[i], k)
    finally:
        r.close()


# ---- 6. more candidates than the mid pipeline's 65 536; the interval routes ---------------------------------------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    """100 000 entries of ten bytes, `a` + one of four bodies of eight + newline: the piece `qrst` hits in three of the
    bodies and `uvwx` in one, 100 000 candidates, of which the exact body's second is dropped as not the first exact piece
    and the body with two substitutions by the count."""
    rng = np.random.default_rng(1560)
    k = 100_000
    bodies = np.array([list(b'qrstuvwx'), list(b'qrstuv#x'), list(b'q#stuv#x'), list(b'qrst#vwx')], dtype=np.uint8)
    which = rng.integers(0, 4, k)
    raw = np.empty((k, 10), dtype=np.uint8)
    raw[:, 0], raw[:, 9] = ord('a'), 0x0A
    raw[:, 1:9] = bodies[which]
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = NearRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, [b'qrstuvwx'], 1, texts=False, order=False)
        assert r.last_stats()['hits'] == int((which != 2).sum() + (which == 0).sum()) > 65536
        assert np.array_equal(np.sort(res.ids), np.flatnonzero(which != 2).astype(np.uint64))
    finally:
        r.close()


@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(1561)
    lines = [filler(rng, int(rng.integers(0, 16))) for _ in range(300)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = NearRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    patterns = []
    while len(patterns) < 520:
        ln = lines[int(rng.integers(0, len(lines)))]
        n = int(rng.integers(6, 9))
        if len(ln) >= n:
            at = int(rng.integers(0, len(ln) - n + 1))
            a = bytearray(ln[at:at + n])
            for i in rng.integers(0, n, int(rng.integers(0, 4))):
                a[int(i)] = FILLER[int(rng.integers(0, 16))]
            patterns.append(bytes(a))
    return p, ref, lines, patterns


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """520 patterns at k = 3 on one chunk are 2 080 pieces and take the 16-lane interval search; the switches force the
    other two.  (The reference of the batch is computed once and shared by the three.)"""
    p, ref, lines, patterns = shape_index
    search_env(**env)
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, patterns, 3, interval=R[route])
        assert res.ids.size >= 520 and (res.counts > 0).sum() > 400
    finally:
        r.close()


# ---- 7. placement ---------------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(1570)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = NearRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'abcd', b'HEAD0', b'HEAD1', b'EAD12', b'ponm', b'MISSING', b'HEAD 0', b'D012 ', b'mnopab']
    patterns += [ch.entry(0)[:9] for ch in ref.chunks if len(ch.entry(0)) >= 4]                      # the entry at offset 0 of every chunk
    patterns += [lines[int(i)][1:8] for i in rng.integers(0, len(lines), 20) if len(lines[int(i)]) >= 8]
    ks = [int(rng.integers(0, 3)) for _ in patterns]
    # devices=[0, 0]: the merge is part-major inside a pattern, so the stated order is not compared there
    base = H.placement(H.NEAR, p, (patterns, ks), search_env, order_multi=False, ref=ref)
    assert base.ids.size > 100 and np.unique(base.ids >> np.uint64(32)).size >= 5


def test_an_empty_chunk_list_and_an_empty_batch():
    r = device_reader([])
    try:
        ref = NearRef([])
        assert r.num_chunks == 0
        res = check(r, ref, [b'error', b'12', b'x\ny'], [1, 1, 2])
        assert res.ids.size == 0 and res.counts.tolist() == [0, 0, 0]
        res = check(r, ref, [], 1)
        assert res.ids.size == 0 and res.counts.size == 0
    finally:
        r.close()
    r, ref, data = one_chunk([b'Error', b'x'])
    try:
        res = check(r, ref, [], 2)
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_near_batch_packed([], 1).offsets.tolist() == [0] and r.count_near_bytes([], []) == []
        # a pattern that a newline voids: no hit is looked at, however often its pieces occur
        got = check(r, ref, [b'r\nx', b'Er\nor'], [1, 2])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
    finally:
        r.close()


# ---- 8. errors and the conveniences ---------------------------------------------------------------------------------------

def test_errors(shape_index):
    p, ref, lines, _ = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        calls = (r.search_near_batch_packed, r.search_near_ids_batch, r.count_near_bytes)
        for call in calls:
            for bad in ([b''], [b'ab', b''], [bytearray()]):
                with pytest.raises(ValueError, match='empty'):
                    call(bad, 0)
            for bad, k in (([b'a'], 1), ([b'abcd', b'abc'], 3), ([b'abcd', b'ab'], [3, 2])):
                with pytest.raises(ValueError, match='every window'):
                    call(bad, k)
            for k in (4, -1, [1, 4], [1], [1, 1, 1]):
                with pytest.raises(ValueError):
                    call([b'abcdef', b'abcdef'], k)
            for bad in (b'ab', 'ab', ['ab'], [None]):
                with pytest.raises(TypeError):
                    call(bad, 1)
            with pytest.raises(TypeError):
                call([b'abcdef'], 1.0)
        # through the C ABI with a reader: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        for blob, offs, ks, what in ((b'abc', [0, 2, 2, 3], [0, 0, 0], 'pattern 1 is empty'), (b'abcdef', [0, 2, 4, 6], [1, 2, 1], 'pattern 1 has 2 bytes'),
                                     (b'abcdef', [0, 2, 4, 6], [1, 1, 4], 'pattern 2 has a budget of 4')):
            offs, ks = np.array(offs, dtype=np.uint64), np.array(ks, dtype=np.uint8)
            for fn in (_ffi.lib.pss_reader_search_near_batch, _ffi.lib.pss_reader_search_near_ids_batch):
                out = ctypes.c_void_p()
                assert fn(h, blob, offs.ctypes.data, 3, ks.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value and what in _ffi.last_error()
                assert fn(h, blob, offs.ctypes.data, 3, ks.ctypes.data, None) == _ffi.PSS_EINVAL
            counts = np.full(4, 7, dtype=np.uint64)
            assert _ffi.lib.pss_reader_count_near_batch(h, blob, offs.ctypes.data, 3, ks.ctypes.data, counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
        # ... and a good batch goes through the same call; the reader still answers
        offs, ks = np.array([0, 2, 3], dtype=np.uint64), np.array([1, 0], dtype=np.uint8)
        out = ctypes.c_void_p()
        assert _ffi.lib.pss_reader_search_near_batch(h, b'abc', offs.ctypes.data, 2, ks.ctypes.data, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == ref.search_near_ids(b'ab', 1).size + ref.search_near_ids(b'c', 0).size > 0
        _ffi.lib.pss_result_free(out)
        # a pattern with a newline: a count of 0, not an error
        assert r.count_near_bytes([b'a\nb', b'ab', b'\n'], 0) == [0, ref.search_near_ids(b'ab', 0).size, 0]
        check(r, ref, [b'abc', b'a\nb', b'cde'], 1)
    finally:
        r.close()


def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    for e in ('password', 'passw0rd!', 'my p@ssw0rd', 'pass word', 'drowssap', 'Été court'):
        w.add_entry(e)
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert sorted(r.search_near('password')) == ['passw0rd!', 'password'] == sorted(r.search_near('password', 1))
        assert sorted(r.search_near('password', 2)) == ['my p@ssw0rd', 'passw0rd!', 'password']
        assert r.search_near('password', 0) == r.search('password') == ['password']
        assert r.count_near('password', 2) == 3 and r.count_near('password') == 2 and r.count_near('pass\nword') == 0
        # a budget counts BYTES: `È` for `É` is one substituted byte, `E` for `É` is a byte fewer -- a deletion, not a substitution
        assert r.search_near('Èté court', 1) == ['Été court'] and r.search_near('Ete court', 2) == [] and r.count_near('Ete', 1) == 0
        for bad in (b'password', [b'password'], ['password'], None):
            with pytest.raises(TypeError):
                r.search_near(bad)
            with pytest.raises(TypeError):
                r.count_near(bad)
        for call in (r.search_near, r.count_near):
            with pytest.raises(ValueError):
                call('')
            with pytest.raises(ValueError):
                call('abc', 3)
            with pytest.raises(ValueError):
                call('abcdef', 4)
            with pytest.raises(TypeError):
                call('abcdef', [1])
    finally:
        r.close()


def test_rows_and_pattern_bytes_around_a_multiple_of_64():
    """63, 64 and 65 patterns whose bytes add up to 31, 32 and 33 modulo 64, budgets 0 and 1 in turn, on one chunk and on three
    (search_harness.layout_edges)."""
    H.layout_edges(H.NEAR, lambda groups: ([ab for _, _, ab in groups], [i % 2 for i in range(len(groups))]), min_ids=63)
