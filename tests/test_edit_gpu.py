"""Search within k edits (Reader.search_near_ids_batch / search_near_batch_packed / count_near_bytes with edits=True, and
the str conveniences) against the brute-force reference of tests/edit_ref.py -- a Sellers scan over every true entry.
Every pattern of every batch goes through one check(), the one of tests/search_harness.py under its EDIT kind:
  * per pattern, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk by the piece index j of each entry's kept candidate
    (d, j) -- the standing candidate with the smallest d, then the smallest j --, inside one piece by the suffix at d;
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result, and every entry's text is the
    reference's for its id;
  * `hits` is the sum of the pieces' exact occurrences (edit_ref.piece_hits);
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), nothing else.
The cases: k and k + 1 edits of every kind on either side of each piece in turn; matches flush with the chunk's ends, which
a fixed window would lose; the newline as a wall; the dedupe at every lane and byte of its first step and past it;
pattern lengths 1 .. 26 at every alignment; 0x00 and high bytes; mixed budgets, k = 0 and the superset of the Hamming
answer; more candidates than the mid pipeline holds; the interval routes; placement; empty inputs; errors; the README's
example."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, near_pieces
from tests import search_harness as H
from tests.edit_ref import EditRef
from tests.search_harness import FILLER, R, device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu

WORD = b'qrstuvwxyz1234567890QRSTUVWXYZ'          # (no byte of the filler, no byte twice)


def check(r, ref, patterns, k, **kw):
    """patterns within k edits (one int, or one per pattern) on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.EDIT, r, ref, (list(patterns), k), **kw)


def one_chunk(lines, closed=True):
    return H.one_chunk(EditRef, lines, closed)


def edited(p, ops):
    """p after the edits ops = [(kind, i)]: 'sub' replaces p[i] by `#`, 'del' drops p[i], 'ins' puts a `#` in front of p[i]
    (i = len(p): behind the last byte).  Applied right to left, so every i is an index of p itself."""
    a = bytearray(p)
    assert b'#' not in p
    for kind, i in sorted(ops, key=lambda o: -o[1]):
        if kind == 'sub':
            a[i] = ord('#')
        elif kind == 'del':
            del a[i]
        else:
            a.insert(i, ord('#'))
    return bytes(a)


# ---- 1. what matches and what does not ----------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_k_edits_of_every_kind_on_either_side_of_each_piece(k):
    """Per piece j in turn the exact one: k edits -- insertions, deletions, substitutions, or the three mixed -- placed left of
    the piece, right of it, or on both sides; beside each plant the same with k + 1 edits.  The reference decides which
    match (an edit at the pattern's rim may be free: a substring is what matches); both classes are non-empty."""
    rng = np.random.default_rng(1720 + k)
    P = WORD[:11 + k]
    cut = near_pieces(P, k)
    lines, planted = [], []
    for j, (off, piece) in enumerate(cut):
        left, right = list(range(0, off)), list(range(off + len(piece) + 1, len(P)))
        if k == 0:          # (the one piece is the pattern: an edit falls inside it and leaves no candidate at all)
            left = list(range(1, len(P) - 1))
        for side in ('left', 'right', 'both'):
            for kinds in (('ins',), ('del',), ('sub',), ('ins', 'del', 'sub')):
                for e in (k, k + 1):
                    for _ in range(2):
                        nl = {'left': e, 'right': 0, 'both': e // 2}[side]
                        if nl > len(left) or e - nl > len(right) or (side == 'both' and (nl == 0 or e - nl == 0)):
                            continue
                        at = rng.choice(left, nl, replace=False).tolist() + rng.choice(right, e - nl, replace=False).tolist()
                        body = edited(P, [(kinds[int(rng.integers(0, len(kinds)))], int(i)) for i in at])
                        assert k == 0 or piece in body
                        planted.append(len(lines))
                        lines.append(filler(rng, int(rng.integers(0, 20))) + body + filler(rng, int(rng.integers(0, 20))))
    planted.append(len(lines))
    lines.append(P)
    lines += [filler(rng, int(rng.integers(0, 40))) for _ in range(30)]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [P], k)
        got = set(res.ids.tolist())
        assert got <= set(planted)
        if k:
            assert len(got) >= 6 * (k + 1) and len(set(planted) - got) >= 6, (len(got), len(planted))
            assert r.last_stats()['hits'] > r.last_stats()['entries']
        else:
            assert len(got) >= 2 and len(set(planted) - got) >= 3
    finally:
        r.close()


def test_repeated_and_nested_pieces_and_short_entries():
    lines = [b'abab', b'abax', b'xbab', b'abxb', b'axab', b'xxab', b'abxx', b'ab', b'aba', b'ababab', b'xabab', b'ababx', b'bababa', b'abb', b'bab',
             b'aaaa', b'aaa', b'a', b'aaab', b'xxxa', b'axxx', b'xxxx', b'xaxx', b'a' * 73, b'aa', b'aabaa', b'aabxa', b'xabaa', b'aaxaa', b'aab', b'baa',
             b'aaaab', b'aabaabaa', b'', b'b', b'b' * 32, b'abcabc', b'abcabd', b'abdabc', b'xbcabc', b'abcxbc', b'abcbc', b'abcaabc', b'x', b'xa', b'ax']
    r, ref, data = one_chunk(lines)
    try:
        patterns = [(b'abab', 1), (b'aaaa', 3), (b'aaaa', 1), (b'aaaa', 0), (b'aabaa', 1), (b'aab', 1), (b'aaa', 2), (b'abcabc', 1), (b'abcabc', 2),
                    (b'a', 0), (b'ab', 1), (b'bbbb', 2), (b'bb', 1), (b'abcabc', 3), (b'aabaa', 2)]
        assert near_pieces(b'abab', 1) == [(0, b'ab'), (2, b'ab')] and near_pieces(b'aab', 1) == [(0, b'a'), (1, b'ab')]
        res = per_pattern(check(r, ref, [p for p, _ in patterns], [k for _, k in patterns]))
        texts = lambda ids: set(r.entries_by_id(ids))
        assert {b'abab', b'abax', b'xbab', b'abxb', b'axab', b'aba', b'abb', b'bab', b'ababab'} <= texts(res[0])
        assert not {b'xxab', b'abxx', b'ab', b'aaaa'} & texts(res[0])
        # `aaaa` within 3: every entry that holds an `a` (three deletions leave one)
        assert texts(res[1]) == {e for e in lines if b'a' in e}
        assert {b'a', b'xa', b'ax', b'b', b'bab'} <= texts(res[10]) and b'x' not in texts(res[10]) and b'' not in texts(res[10])
    finally:
        r.close()


# ---- 2. the chunk's ends and the newline ---------------------------------------------------------------------------------

def test_matches_flush_with_the_chunk_ends():
    """What the fixed window's reject would lose.  `qrtuvwx` at a chunk's start: the piece `uvwx` stands at d = 3 < off = 4.
    `qrstuvx` at a chunk's end, closed and unterminated, and `qrstuvwx12` for `qrstuvwxyz12`: d - off + L > n.  One-byte and
    two-byte entries and chunks."""
    P, Q = b'qrstuvwx', b'qrstuvwxyz12'
    texts = [b'qrtuvwx opens\nnothing\nat the end qrstuvx',       # 0: a deletion left of `uvwx` at the start, right of `qrst` at the unterminated end
             b'qrtuvwx\nnothing\nqrstuvx\n',                        # 1: the same, closed, the entries nothing but the match
             b'qtuvwxyz12\nqrstuvwx12\n',                           # 2: two deletions, k = 2
             b'qtuvwxyz12 and\nthen qrstuvwx12',                    # 3
             b'q', b'qr', b'r\n', b'x\nqr\nq\n', b'x', b'rs',       # 4 .. 9
             b'qrstuvw', b'rstuvwx', b'qrstuvwx',                   # 10 .. 12: a byte short at either end, and the pattern itself
             b'uvwx', b'qrst\nuvwx\n']                              # 13, 14: one piece alone
    r, ref = device_reader(texts), EditRef(texts)
    try:
        res = per_pattern(check(r, ref, [P, P, Q, Q, b'qr', b'qrs', b'q', P], [1, 0, 2, 1, 1, 2, 0, 2]))
        one = res[0].tolist()
        assert {0, (0 << 32) | 2, 1 << 32, (1 << 32) | 2, 10 << 32, 11 << 32, 12 << 32} <= set(one)
        assert not {13 << 32, 14 << 32, (14 << 32) | 1} & set(one)
        assert res[1].tolist() == [(2 << 32) | 1, (3 << 32) | 1, 12 << 32]
        assert {2 << 32, (2 << 32) | 1, 3 << 32, (3 << 32) | 1} <= set(res[2].tolist()) and not {2 << 32, (2 << 32) | 1} & set(res[3].tolist())
        # `qr` within 1: every entry that holds a `q` or an `r`
        assert {4 << 32, 5 << 32, 6 << 32, (7 << 32) | 1, (7 << 32) | 2, 9 << 32} <= set(res[4].tolist())
        assert 8 << 32 not in res[4].tolist() and 7 << 32 not in res[4].tolist()
        assert {4 << 32, 5 << 32, 6 << 32, 9 << 32} <= set(res[5].tolist())
    finally:
        r.close()
    # 0x00 as a pattern's last byte next to the chunk's end: the zero padding behind n is not text
    texts0 = [b'ab\x00', b'ab', b'xab\nab\x00\x00', b'a\x00\x00', b'ab\x00\x00']
    r0, ref0 = device_reader(texts0), EditRef(texts0)
    try:
        res = per_pattern(check(r0, ref0, [b'ab\x00', b'ab\x00\x00', b'ab\x00\x00', b'b\x00\x00\x00', b'\x00\x00', b'ab\x00\x00\x00'], [0, 0, 1, 1, 1, 1]))
        assert res[0].tolist() == [0, (2 << 32) | 1, 4 << 32] and res[1].tolist() == [(2 << 32) | 1, 4 << 32]
        assert 1 << 32 not in res[2].tolist() and 0 in res[2].tolist()
        assert res[5].tolist() == [(2 << 32) | 1, 4 << 32]
    finally:
        r0.close()


def test_a_match_that_needs_the_newline_among_its_edits_is_none():
    for closed in (True, False):
        lines = [b'pass', b'word', b'xxpass', b'wordxx', b'password', b'pasword', b'xpas', b'sword', b'', b'pass', b'', b'word', b'pas', b'word',
                 b'yyyypassw', b'ord']
        r, ref, data = one_chunk(lines, closed)
        try:
            assert data.startswith(b'pass\nword') and data.rstrip(b'\n').endswith(b'passw\nord')
            res = per_pattern(check(r, ref, [b'password'] * 4 + [b'pass\nword', b's\nw'], [0, 1, 2, 3, 1, 1]))
            assert r.entries_by_id(res[0]) == [b'password'] and set(r.entries_by_id(res[1])) == {b'pasword', b'password'} == set(r.entries_by_id(res[2]))
            # (`passw` and `sword` are three deletions away; `pass` + `word` over the newline would be one)
            assert set(r.entries_by_id(res[3])) == {b'pasword', b'password', b'yyyypassw', b'sword'}
            assert res[4].size == 0 and res[5].size == 0
            assert r.last_stats()['hits'] > 20
        finally:
            r.close()


# ---- 3. the dedupe --------------------------------------------------------------------------------------------------------

def test_entries_that_hold_the_pattern_several_times():
    rng = np.random.default_rng(1730)
    P = WORD[:12]
    forms = [P, edited(P, [('del', 5)]), edited(P, [('ins', 7)]), edited(P, [('sub', 1), ('del', 9)]), edited(P, [('sub', 2), ('sub', 6), ('sub', 10)])]
    lines = []
    for a in forms:
        for b in forms:
            for gap in (0, 1, 3, 40, 70, 140):
                lines.append(filler(rng, int(rng.integers(0, 9))) + a + filler(rng, gap) + b + filler(rng, int(rng.integers(0, 9))))
    lines += [P * 5, P[:8] * 6, (P + b'#') * 4]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [P] * 4, [0, 1, 2, 3])
        assert res.counts.tolist()[3] >= len(lines) - 1 and res.counts.tolist()[0] >= 2 * 6
        assert r.last_stats()['hits'] > 2 * r.last_stats()['entries']
    finally:
        r.close()


@pytest.mark.parametrize('length', [63, 64, 65, 71, 72, 129])
def test_an_earlier_standing_candidate_at_every_lane_and_byte(length):
    """An exact `qrstu` at the entry's end and, in front of it, at every position of the first 64-byte step and one past it
    (as far as the entry reaches), a form of the pattern within budget -- the hit at the end is dropped, the entry still
    comes once, kept at the earlier candidate -- or beyond it, which changes nothing."""
    rng = np.random.default_rng(1740 + length)
    P = b'qrstu'
    lines = []
    for at in range(0, min(66, length - 11)):
        for first in (b'qrtu', b'qr#stu', b'q#stu', b'q#t#', b'#rs#u'):
            e = bytearray(filler(rng, length))
            e[at:at + len(first)], e[length - 5:] = first, P
            assert len(e) == length
            lines.append(bytes(e))
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [P, P, P], [1, 2, 0])
        assert res.counts.tolist() == [len(lines)] * 3
        # (within 1 the entries of `qrtu`, `qr#stu` and `q#stu` are kept at the earlier candidate, through its piece `qr` or `stu` / `tu`;
        # the entries of the other two at the exact occurrence: check() has held the order of both against the reference)
        assert np.array_equal(per_pattern(res)[0], ref.ordered_ids(P, 1))
    finally:
        r.close()


# ---- 4. load widths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_pattern_lengths_1_to_26_at_every_alignment(k):
    """Every pattern length k + 1 .. 26, planted with the last piece exact at every alignment of d against the 8-byte word:
    one deletion in each other piece (a match), and those with one substitution in the last piece too (no candidate there)."""
    rng = np.random.default_rng(1750 + k)
    lines, patterns = [], []

    def add(body, d, lead):         # body in an entry of its own, its byte d at an offset of the chunk that is lead mod 8
        at = sum(len(x) + 1 for x in lines)
        lines.append(b'#' * ((lead - at - d) % 8) + body)

    for L in range(k + 1, 27):
        P = WORD[:L]
        cut = near_pieces(P, k)
        ops = [('del', off + len(piece) - 1) for off, piece in cut[:-1] if len(piece) > 1] + [('sub', off) for off, piece in cut[:-1] if len(piece) == 1]
        within = edited(P, ops)
        beyond = edited(P, ops + [('sub', L - 1)])
        patterns.append(P)
        for lead in range(8):
            add(within + filler(rng, int(rng.integers(0, 6))), within.index(cut[-1][1]), lead)
            add(beyond, 0, lead)
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, patterns, k)
        assert (res.counts >= 8).all()
    finally:
        r.close()


# ---- 5. bytes, budgets and k = 0 -------------------------------------------------------------------------------------------

def test_zero_and_high_bytes_are_bytes_like_any_other():
    rng = np.random.default_rng(1760)
    abc = np.frombuffer(b'\x00\x80\xff\xc3\xa9\x7f\x01', np.uint8)
    lines = [bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 24)))]) for _ in range(200)]
    lines += [b'\x00' * 9, b'\xff' * 9, b'\x00\x00\x00', b'caf\xc3\xa9', b'caf\xc3\xa8', b'cafe', b'caf\xa9', b'c\xc3\xa9']
    r, ref, data = one_chunk(lines, closed=False)
    try:
        patterns = [b'\x00\x00', b'\x00\x80\xff', b'\xff\xff\xff\xff', b'\xc3\xa9', b'caf\xc3\xa9', b'\x00' * 9, b'\x80\x00\x80\x00\x80', b'\x7f\x01\x00\x00']
        for k in (0, 1, 2):
            check(r, ref, [p for p in patterns if len(p) > k], k)
        res = per_pattern(check(r, ref, [b'caf\xc3\xa9', b'caf\xc3\xa9'], [0, 1]))
        assert r.entries_by_id(res[0]) == [b'caf\xc3\xa9']
        assert sorted(r.entries_by_id(res[1])) == [b'caf\xa9', b'caf\xc3\xa8', b'caf\xc3\xa9']      # (a byte fewer is ONE edit; `cafe` is two)
    finally:
        r.close()


def test_mixed_budgets_k_zero_and_the_hamming_answer():
    rng = np.random.default_rng(1761)
    lines = [filler(rng, int(rng.integers(0, 30))) for _ in range(300)]
    r, ref, data = one_chunk(lines)
    try:
        patterns = [b'a', b'ab', b'abc', b'mnop', b'pon', b'zz', b'abcdefgh', b'ponmlk', b'p', b'hgf']
        patterns += [lines[int(i)][1:int(rng.integers(3, 12))] for i in rng.integers(0, len(lines), 24) if len(lines[int(i)]) >= 12]
        got, plain = check(r, ref, patterns, 0), r.search_ids_batch(patterns)
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts) and got.ids.size > 300
        ks = [min(int(rng.integers(0, 4)), len(p) - 1) for p in patterns]
        assert {0, 1, 2, 3} <= set(ks)
        mixed = check(r, ref, patterns, ks)
        # edits=False is the search within k mismatches, as it was, and its answer is part of the edit answer
        near = r.search_near_ids_batch(patterns, ks)
        again = r.search_near_ids_batch(patterns, ks, edits=False)
        assert np.array_equal(near.ids, again.ids) and np.array_equal(near.counts, again.counts)
        assert r.count_near_bytes(patterns, ks) == near.counts.tolist() == r.count_near_bytes(patterns, ks, edits=False)
        more = 0
        for p, kk, e, h in zip(patterns, ks, per_pattern(mixed), per_pattern(near)):
            assert set(h.tolist()) <= set(e.tolist()), (p, kk)
            more += e.size > h.size
        assert more >= 5
        for k in range(4):          # every pattern of the mixed batch: what a batch of its own budget returns
            some = [i for i, kk in enumerate(ks) if kk == k]
            alone = per_pattern(check(r, ref, [patterns[i] for i in some], k))
            for i, ids in zip(some, alone):
                assert np.array_equal(per_pattern(mixed)[i], ids), (patterns[i], k)
    finally:
        r.close()


# ---- 6. more candidates than the mid pipeline's 65 536; the interval routes ---------------------------------------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    """100 000 entries, `a` + one of five bodies + newline: the piece `qrst` hits in four of the bodies and `uvwx` in two."""
    rng = np.random.default_rng(1770)
    k = 100_000
    bodies = [b'qrstuvwx', b'qrstuvx', b'q#stuv#x', b'qrst#uvwx', b'qrst##vwx']
    which = rng.integers(0, len(bodies), k)
    data = b''.join(b'a' + bodies[int(w)] + b'\n' for w in which)
    p = make_index(tmp_path, 'many', data)
    ref = EditRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, [b'qrstuvwx'], 1, texts=False, order=False)
        assert r.last_stats()['hits'] == int((which != 2).sum() + (which == 0).sum() + (which == 3).sum()) > 65536
        assert np.array_equal(np.sort(res.ids), np.flatnonzero(np.isin(which, (0, 1, 3))).astype(np.uint64))
    finally:
        r.close()


@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(1771)
    lines = [filler(rng, int(rng.integers(0, 16))) for _ in range(200)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = EditRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    patterns = []
    while len(patterns) < 520:
        ln = lines[int(rng.integers(0, len(lines)))]
        n = int(rng.integers(7, 10))
        if len(ln) >= n:
            at = int(rng.integers(0, len(ln) - n + 1))
            a = bytearray(ln[at:at + n])
            for _ in range(int(rng.integers(0, 4))):
                i, op = int(rng.integers(0, len(a))), int(rng.integers(0, 3))
                if op == 0:
                    a[i] = FILLER[int(rng.integers(0, 16))]
                elif op == 1 and len(a) > 5:
                    del a[i]
                else:
                    a.insert(i, FILLER[int(rng.integers(0, 16))])
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
    rng = np.random.default_rng(1780)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1000)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 3000)
    ref = EditRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'abcd', b'HEAD0', b'HEAD1', b'EAD12', b'ponm', b'MISSING', b'HEAD 0', b'D012 ', b'mnopab', b'HED04', b'HEEAD00']
    patterns += [ch.entry(0)[1:9] for ch in ref.chunks if len(ch.entry(0)) >= 5]                     # a deletion at offset 0 of every chunk
    patterns += [lines[int(i)][1:8] for i in rng.integers(0, len(lines), 12) if len(lines[int(i)]) >= 8]
    ks = [min(int(rng.integers(0, 3)), len(q) - 1) for q in patterns]
    # devices=[0, 0]: the merge is part-major inside a pattern, so the stated order is not compared there
    base = H.placement(H.EDIT, p, (patterns, ks), search_env, order_multi=False, ref=ref)
    assert base.ids.size > 100 and np.unique(base.ids >> np.uint64(32)).size >= 5


def test_an_empty_chunk_list_and_an_empty_batch():
    r = device_reader([])
    try:
        ref = EditRef([])
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
        assert r.search_near_batch_packed([], 1, edits=True).offsets.tolist() == [0] and r.count_near_bytes([], [], edits=True) == []
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
                    call(bad, 0, edits=True)
            for bad, k in (([b'a'], 1), ([b'abcd', b'abc'], 3), ([b'abcd', b'ab'], [3, 2])):
                with pytest.raises(ValueError, match='deleting all of it'):
                    call(bad, k, edits=True)
            for k in (4, -1, [1, 4], [1], [1, 1, 1]):
                with pytest.raises(ValueError):
                    call([b'abcdef', b'abcdef'], k, edits=True)
            for bad in (b'ab', 'ab', ['ab'], [None]):
                with pytest.raises(TypeError):
                    call(bad, 1, edits=True)
            with pytest.raises(TypeError):
                call([b'abcdef'], 1.0, edits=True)
            with pytest.raises(TypeError):
                call([b'abcdef'], 1, edits=1)
        # through the C ABI with a reader: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        for blob, offs, ks, what in ((b'abc', [0, 2, 2, 3], [0, 0, 0], 'pattern 1 is empty'), (b'abcdef', [0, 2, 4, 6], [1, 2, 1], 'pattern 1 has 2 bytes'),
                                     (b'abcdef', [0, 2, 4, 6], [1, 1, 4], 'pattern 2 has a budget of 4 edits')):
            offs, ks = np.array(offs, dtype=np.uint64), np.array(ks, dtype=np.uint8)
            for fn in (_ffi.lib.pss_reader_search_edit_batch, _ffi.lib.pss_reader_search_edit_ids_batch):
                out = ctypes.c_void_p()
                assert fn(h, blob, offs.ctypes.data, 3, ks.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value and what in _ffi.last_error()
                assert fn(h, blob, offs.ctypes.data, 3, ks.ctypes.data, None) == _ffi.PSS_EINVAL
            counts = np.full(4, 7, dtype=np.uint64)
            assert _ffi.lib.pss_reader_count_edit_batch(h, blob, offs.ctypes.data, 3, ks.ctypes.data, counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
        # ... and a good batch goes through the same call; the reader still answers
        offs, ks = np.array([0, 2, 3], dtype=np.uint64), np.array([1, 0], dtype=np.uint8)
        out = ctypes.c_void_p()
        assert _ffi.lib.pss_reader_search_edit_batch(h, b'abc', offs.ctypes.data, 2, ks.ctypes.data, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == ref.search_edit_ids(b'ab', 1).size + ref.search_edit_ids(b'c', 0).size > 0
        _ffi.lib.pss_result_free(out)
        # a pattern with a newline: a count of 0, not an error
        assert r.count_near_bytes([b'a\nb', b'ab', b'\n'], 0, edits=True) == [0, ref.search_edit_ids(b'ab', 0).size, 0]
        check(r, ref, [b'abc', b'a\nb', b'cde'], 1)
    finally:
        r.close()


def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    for e in ('password', 'passw0rd!', 'my pasword', 'passsword', 'pass-word', 'pass word', 'psswrd', 'drowssap', 'Été court'):
        w.add_entry(e)
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert sorted(r.search_near('password', k=1, edits=True)) == ['my pasword', 'pass word', 'pass-word', 'passsword', 'passw0rd!', 'password']
        assert sorted(r.search_near('password', 1)) == ['passw0rd!', 'password'] == sorted(r.search_near('password', 1, edits=False))
        assert sorted(r.search_near('password', 2, True)) == sorted(r.search_near('password', k=1, edits=True) + ['psswrd'])
        assert r.search_near('password', 0, edits=True) == r.search('password') == ['password']
        assert r.count_near('password', 1, edits=True) == 6 and r.count_near('password') == 2 and r.count_near('pass\nword', edits=True) == 0
        # a budget counts BYTES: `Ete` for `Été` is three edits -- `t` stays, and on either side of it one byte of two
        assert r.search_near('Ete court', 3, edits=True) == ['Été court'] and r.search_near('Ete court', 2, edits=True) == []
        for bad in (b'password', [b'password'], ['password'], None):
            with pytest.raises(TypeError):
                r.search_near(bad, edits=True)
            with pytest.raises(TypeError):
                r.count_near(bad, edits=True)
        for call in (r.search_near, r.count_near):
            with pytest.raises(ValueError):
                call('', edits=True)
            with pytest.raises(ValueError):
                call('abc', 3, edits=True)
            with pytest.raises(ValueError):
                call('abcdef', 4, edits=True)
            with pytest.raises(TypeError):
                call('abcdef', [1], edits=True)
            with pytest.raises(TypeError):
                call('abcdef', 1, edits='yes')
    finally:
        r.close()


def test_rows_and_pattern_bytes_around_a_multiple_of_64():
    """63, 64 and 65 patterns whose bytes add up to 31, 32 and 33 modulo 64, budgets 0 and 1 in turn, on one chunk and on three
    (search_harness.layout_edges)."""
    H.layout_edges(H.EDIT, lambda groups: ([ab for _, _, ab in groups], [i % 2 for i in range(len(groups))]), min_ids=63)
