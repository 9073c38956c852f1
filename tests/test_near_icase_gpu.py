"""Search within k mismatches and within k edits under ASCII case folding (Reader.search_near_ids_batch /
search_near_batch_packed / count_near_bytes with icase=True, with and without edits=True, and the str conveniences) against
the brute-force references of tests/near_icase_ref.py: both sides folded, then the window count or the Sellers scan.
Every pattern of every batch goes through the one check() of tests/search_harness.py, under two kinds defined here:
  * per pattern, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk by the piece index of the kept hit, then by query (the
    spellings of a seed ascend bytewise) and in suffix-array order;
  * entry by entry, entries_by_id_packed(ids) is the packed text result, and every entry's text is the reference's;
  * `hits` is the sum of the exact occurrences of every seed query (near_icase_ref.piece_hits);
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), nothing else.
The cases follow DESIGN.md 4.19: k and k + 1 substitutions under flipped case; the bytes that must not fold; pieces over
the letter cap with the seed inside its piece; pieces without letters; pieces that repeat or nest under fold only; one-byte
entries; the newline; both ends of a chunk; both ends of an entry; the dedupe across spellings, at every lane and byte of
its first step; pattern lengths at every alignment; mixed budgets; the three relations of the contract; an edit beside a
case flip; placement and the interval routes; empty inputs; errors."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, near_pieces, near_seeds
from tests import search_harness as H
from tests.near_icase_ref import EditIcaseRef, NearIcaseRef
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu

NEAR = H._near('near_icase', NearIcaseRef, lambda ref, p, k: ref.search_near_ids(p, k), icase=True)
EDIT = H._near('edit_icase', EditIcaseRef, lambda ref, p, k: ref.search_edit_ids(p, k), edits=True, icase=True)
KINDS = pytest.mark.parametrize('kind', [NEAR, EDIT], ids=['mismatches', 'edits'])
WORD = b'qRsTuVwXyZ1234567890QrStUvWxYz'          # (no byte of the filler under fold; letters in both cases, digits)


def check(kind, r, ref, patterns, k, **kw):
    return H.check(kind, r, ref, (list(patterns), k), **kw)


def one_chunk(kind, lines, closed=True):
    return H.one_chunk(kind.ref_cls, lines, closed)


def want(kind, ref, p, k):
    return set(kind.want(ref, p, k).tolist())


def mangled(rng, b):
    """b with the case of each ASCII letter drawn anew."""
    return bytes(c ^ 0x20 if 0x61 <= (c | 0x20) <= 0x7a and rng.random() < 0.5 else c for c in b)


def substituted(p, at):
    a = bytearray(p)
    for i in at:
        a[i] = ord('#')
    return bytes(a)


def edited(p, ops):
    """p after ops = [(kind, i)]: 'sub' replaces p[i] by `#`, 'del' drops p[i], 'ins' puts a `#` in front of p[i]."""
    a = bytearray(p)
    for kind, i in sorted(ops, key=lambda o: -o[1]):
        if kind == 'sub':
            a[i] = ord('#')
        elif kind == 'del':
            del a[i]
        else:
            a.insert(i, ord('#'))
    return bytes(a)


# ---- 1, 2: what matches and what does not ------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_k_substitutions_under_flipped_case(kind, k):
    """The pattern with the case of EVERY letter flipped and exactly k bytes substituted matches; with k + 1 it does not."""
    rng = np.random.default_rng(1930 + k)
    P = WORD[:11 + k]
    lines, within, beyond = [], [], []
    for e, bucket in ((k, within), (k + 1, beyond)):
        for _ in range(12):
            at = rng.choice(np.arange(1, len(P) - 1), e, replace=False).tolist()
            bucket.append(len(lines))
            lines.append(filler(rng, int(rng.integers(0, 20))) + substituted(P.swapcase(), at) + filler(rng, int(rng.integers(0, 20))))
    lines += [filler(rng, int(rng.integers(0, 40))) for _ in range(20)] + [P, P.swapcase(), P.lower(), P.upper()]
    r, ref, data = one_chunk(kind, lines)
    try:
        got = set(check(kind, r, ref, [P], k).ids.tolist())
        assert set(within) <= got and not set(beyond) & got and got >= set(range(len(lines) - 4, len(lines)))
        if k:       # without the keyword none of the flipped ones is found
            exact = set(r.search_near_ids_batch([P], k, edits=kind is EDIT).ids.tolist())
            assert exact < got and not exact & set(within)
    finally:
        r.close()


@KINDS
def test_only_ascii_letters_fold(kind):
    """`@` / '`', `[` / `{` and 0xC9 / 0xE9 are one bit away from each other, as `A` / `a` are, and do not fold: each counts as a
    mismatch.  0x00 is a byte like any other, at the end of an unterminated chunk too."""
    P = b'a@b[c\xc9d'
    forms = [P, P.upper(), b'a`b[c\xc9d', b'a@b{c\xc9d', b'a@b[c\xe9d', b'A`B{C\xc9D', b'A`B{C\xe9D', b'a@b[c\xc9', b'`@[{\xc9\xe9', b'A@B[C\xc9D']
    lines = [b'xx' + f + b'yy' for f in forms] + forms + [b'ab\x00cd', b'AB\x00CD', b'AB CD', b'Ab\x80cD', b'', b'\x00']
    texts = [b'\n'.join(lines) + b'\n', b'zz\nAB\x00', b'ab\x00\x00', b'Ab']
    r, ref = device_reader(texts), kind.ref_cls(texts)
    try:
        res = per_pattern(check(kind, r, ref, [P, P, P, P, b'ab\x00cd', b'ab\x00cd', b'AB\x00', b'ab\x00\x00', b'Ab\x00\x00'], [0, 1, 2, 3, 0, 1, 0, 0, 1]))
        texts0 = lambda ids: [e for e in r.entries_by_id(ids)]
        assert sorted(set(texts0(res[0]))) == sorted({P, P.upper(), b'xx' + P + b'yy', b'xx' + P.upper() + b'yy', b'A@B[C\xc9D', b'xxA@B[C\xc9Dyy'})
        one = set(texts0(res[1]))
        assert {b'a`b[c\xc9d', b'a@b{c\xc9d', b'a@b[c\xe9d'} <= one and not {b'A`B{C\xc9D', b'A`B{C\xe9D'} & one
        assert b'A`B{C\xc9D' in set(texts0(res[2])) and b'A`B{C\xe9D' not in set(texts0(res[2])) and b'A`B{C\xe9D' in set(texts0(res[3]))
        assert set(texts0(res[4])) == {b'ab\x00cd', b'AB\x00CD'}
        assert {b'AB CD', b'Ab\x80cD'} <= set(texts0(res[5]))
        assert res[6].tolist()[-2:] == [(1 << 32) | 1, 2 << 32] and res[7].tolist() == [2 << 32]
        assert 3 << 32 not in res[8].tolist() and 2 << 32 in res[8].tolist()      # (the zero padding behind n is not text)
    finally:
        r.close()


# ---- 3, 4, 5: the seed inside its piece --------------------------------------------------------------------------------------

@KINDS
def test_pieces_over_the_letter_cap(kind):
    """14 letters at k = 1: two pieces of 7 letters, seeds of 5.  16 bytes `abcdefg1hijklmn2`: the seeds `cdefg1` / `jklmn2`
    stand 2 bytes into their pieces.  The piece's bytes outside the seed in the other case; a substitution inside piece 0
    but outside its seed (its hit is rejected, piece 1's kept); the entry at chunk offset 0 with its first bytes missing,
    so that the seed's hit lies nearer to the chunk's start than the seed to the pattern's."""
    A, B = b'abcdefghijklmn', b'abcdefg1hijklmn2'
    assert [(j, pos) for j, pos, _ in near_seeds(A, 1)[::32]] == [(0, 0), (1, 7)] and len(near_seeds(A, 1)) == 64
    assert [(j, pos, q.lower()) for j, pos, q in near_seeds(B, 1)[::32]] == [(0, 2, b'cdefg1'), (1, 10, b'jklmn2')]
    lines = [A, A.upper(), b'ABCDEfgHIJKLmn', b'abcdeFGhijklMN', b'abcde#ghijklmn', b'ABCDEF#HIJKLMN', b'abcdefghijkl#n', b'ab#defghijklmn', b'abcdefg#ijklmn',
             b'abcde#ghijkl#n', b'xxABCDEFGHIJKLMNxx', B, B.swapcase(), b'ABcdefg1HIjklmn2', b'#bcdefg1hijklmn2', b'#Bcdefg1Hijklmn2', b'a#cdefg1hijklmn2',
             b'abcdefg1#ijklmn2', b'abcdefg1h#jklmn2', b'#bcdefg1#ijklmn2', b'bcdefg1hijklmn2', b'abcdefg1hijklmn', b'abcdefg1ijklmn2', b'abcdefg1hhijklmn2']
    texts = [b'BCDEFG1hijklmn2\n' + b'\n'.join(lines) + b'\n', b'cdefg1HIJKLMN2\nx', b'#Bcdefg1hijklmN2', b'fg1hijklmn2\n', b'Abcdefg1hijklmn', b'hijklmn\n', b'ABCDEFG']
    r, ref = device_reader(texts), kind.ref_cls(texts)
    try:
        res = per_pattern(check(kind, r, ref, [A, B, A, B, A, B], [1, 1, 2, 2, 0, 3]))
        assert {b'abcde#ghijklmn', b'ABCDEF#HIJKLMN', b'abcdefghijkl#n', b'ab#defghijklmn', b'ABCDEfgHIJKLmn'} <= set(r.entries_by_id(res[0]))
        assert b'abcde#ghijkl#n' not in r.entries_by_id(res[0]) and b'abcde#ghijkl#n' in r.entries_by_id(res[2])
        found = set(res[1].tolist())
        assert 2 << 32 in found and {b'#bcdefg1hijklmn2', b'#Bcdefg1Hijklmn2', b'ABcdefg1HIjklmn2'} <= set(r.entries_by_id(res[1]))
        if kind is EDIT:        # a byte short at the chunk's start and at its end; two bytes short, the seed flush with the start
            assert {0, 4 << 32} <= found and 1 << 32 not in found and 1 << 32 in set(res[3].tolist())
        else:
            assert not {0, 1 << 32, 3 << 32, 4 << 32} & found
    finally:
        r.close()


@KINDS
def test_pieces_without_letters_and_pieces_that_repeat_or_nest_under_fold_only(kind):
    lines = [b'abab', b'ABAB', b'AbaB', b'abax', b'XBAB', b'aBxb', b'AXab', b'xxAB', b'ABxx', b'ab', b'aBa', b'abABab', b'xAbAbx', b'BABABA', b'Abb', b'bAb',
             b'aAb', b'AAB', b'aab', b'aAx', b'xAb', b'Aa', b'aA', b'AABAA', b'aabxA', b'a', b'A', b'b', b'B', b'', b'x', b'Xa', b'aX',
             b'1234abcd5678', b'1234ABCD5678', b'1234AB#D5678', b'12#4ABCD5678', b'1234aBcD56#8', b'1#34abcd567#', b'1234#BCD#678', b'12345678', b'1234abcd567',
             b'234abcd5678', b'1234abd5678', b'1234ab-cd5678']
    r, ref, data = one_chunk(kind, lines, closed=False)
    try:
        assert near_pieces(b'AbaB', 1) == [(0, b'Ab'), (2, b'aB')] and near_pieces(b'aAb', 1) == [(0, b'a'), (1, b'Ab')]
        assert [q for _, _, q in near_seeds(b'1234abcd5678', 2)] == [b'1234'] + sorted(bytes(x) for x in {b'ABCD', b'ABCd', b'ABcD', b'ABcd', b'AbCD', b'AbCd',
                b'AbcD', b'Abcd', b'aBCD', b'aBCd', b'aBcD', b'aBcd', b'abCD', b'abCd', b'abcD', b'abcd'}) + [b'5678']
        patterns = [(b'AbaB', 1), (b'aAb', 1), (b'AbaB', 0), (b'aAb', 0), (b'AbaB', 2), (b'aAbAa', 1), (b'1234abcd5678', 2), (b'1234ABCD5678', 1),
                    (b'1234abcd5678', 3), (b'a', 0), (b'A', 0), (b'aB', 1), (b'12345678', 1), (b'Ab', 0), (b'bA', 1)]
        res = per_pattern(check(kind, r, ref, [p for p, _ in patterns], [k for _, k in patterns]))
        texts = lambda ids: set(r.entries_by_id(ids))
        assert {b'abab', b'ABAB', b'AbaB', b'abax', b'XBAB', b'aBxb', b'AXab', b'abABab'} <= texts(res[0]) and not {b'xxAB', b'ABxx', b'ab'} & texts(res[0])
        assert {b'aAb', b'AAB', b'aab', b'aAx', b'xAb', b'AABAA'} <= texts(res[1])
        assert {b'1234abcd5678', b'1234ABCD5678', b'1234AB#D5678', b'12#4ABCD5678', b'1234aBcD56#8', b'1#34abcd567#', b'1234#BCD#678'} <= texts(res[6])
        assert texts(res[9]) == texts(res[10]) >= {e for e in lines[:-1] if b'a' in e.lower()}
        assert ({b'a', b'A', b'b', b'B'} <= texts(res[11])) == (kind is EDIT) and b'' not in texts(res[11]) and b'x' not in texts(res[11])
        assert {b'aX', b'ab', b'bAb'} <= texts(res[11])
    finally:
        r.close()


# ---- 7, 8, 9: the newline, the chunk's ends, the entry's ends ----------------------------------------------------------------

@KINDS
def test_the_newline_and_both_ends_of_chunks_and_entries(kind):
    P, Q = b'qRsTuVwX', b'QrStUvWxYz12'
    texts = [b'QRTUVWX opens\nnothing\nat the end qrstuvx',        # a deletion at the chunk's start and at its unterminated end
             b'qrtuvwx\nnothing\nQRSTUVX\n',
             b'qRSTUVWX and\nthen QRSTUVWx',                        # the pattern flush with both ends of the chunk, in other spellings
             b'RSTUVWX', b'qrstuvw', b'QRSTUVWX', b'q', b'Qr', b'R\n', b'x\nqR\nQ\n', b'x',
             b'Pass\nWORD\nxxPASS\nwordxx\nPassWord\nPASWORD\npass\n\nword\nyyyyPASSW\nord',
             b'uvwx', b'QRST\nUVWX\n', b'#RSTUVWX\nQRSTUVW#\nQRSTUVW\nRSTUVWX\nxQRSTUVWXx\nQ#STUVWX\nQRSTUV#X',
             b'stuvwxyz12\nQRSTUVWXYZ', b'TuVwXyZ12']
    r, ref = device_reader(texts), kind.ref_cls(texts)
    try:
        res = per_pattern(check(kind, r, ref, [P, P, P, Q, Q, b'qR', b'Q', b'password', b'PASSWORD', b'pass\nword', b'S\nW', Q],
                                [1, 0, 2, 2, 1, 1, 0, 1, 3, 1, 1, 3]))
        one = set(res[0].tolist())
        assert {2 << 32, (2 << 32) | 1, 5 << 32, 14 << 32, (14 << 32) | 1, (14 << 32) | 4, (14 << 32) | 5, (14 << 32) | 6} <= one
        assert res[1].tolist() and set(res[1].tolist()) == {2 << 32, (2 << 32) | 1, 5 << 32, (14 << 32) | 4, (15 << 32) | 1}
        assert not {12 << 32, 13 << 32, (13 << 32) | 1} & one
        assert ({0, (0 << 32) | 2, 1 << 32, (1 << 32) | 2, 3 << 32, 4 << 32, (14 << 32) | 2, (14 << 32) | 3} <= one) == (kind is EDIT)
        assert (15 << 32 in res[3].tolist()) == (kind is EDIT) and ((15 << 32) | 1 in res[3].tolist()) == (kind is EDIT)
        assert (16 << 32 in res[11].tolist()) == (kind is EDIT)
        assert set(r.entries_by_id(res[7])) == ({b'PassWord', b'PASWORD'} if kind is EDIT else {b'PassWord'})
        assert b'pass' not in r.entries_by_id(res[8]) and b'WORD' not in r.entries_by_id(res[8])
        assert res[9].size == 0 and res[10].size == 0
    finally:
        r.close()


# ---- 10, 11, 12: the dedupe -----------------------------------------------------------------------------------------------------

@KINDS
def test_an_entry_comes_once_whatever_spellings_it_holds(kind):
    rng = np.random.default_rng(1940)
    P = WORD[:12]
    forms = [P, P.swapcase(), P.upper(), substituted(P.lower(), [5]), edited(P.upper(), [('del', 5)]), edited(P.swapcase(), [('ins', 7)]),
             substituted(P.swapcase(), [2, 9])]
    lines = []
    for a in forms:
        for b in forms:
            for gap in (0, 1, 40, 70, 140):
                lines.append(filler(rng, int(rng.integers(0, 9))) + a + filler(rng, gap) + b + filler(rng, int(rng.integers(0, 9))))
    lines += [P + P.upper() + P.lower(), P.lower() + b' ' + P.swapcase() + b' ' + P, (P.upper() + b'#') * 4, mangled(rng, P[:8] * 6)]
    r, ref, data = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, [P] * 4, [0, 1, 2, 3])
        assert res.counts.tolist()[0] >= 3 * 7 * 5 and res.counts.tolist()[2] >= (len(lines) - 1 if kind is EDIT else 225)
        assert r.last_stats()['hits'] > 2 * r.last_stats()['entries']
        # an earlier window within budget, in another spelling, drops the later hit: the kept hit's suffix says which
        assert np.array_equal(per_pattern(res)[1], ref.ordered_ids(P, 1))
    finally:
        r.close()


@KINDS
@pytest.mark.parametrize('length', [63, 64, 65, 127, 128])
def test_an_earlier_match_at_every_lane_and_byte(kind, length):
    """The pattern at the entry's end and, in front of it, at every position of the first 64-byte step and one past it (as far
    as the entry reaches), another spelling of it within budget -- the hit at the end is dropped, the entry comes once, kept
    at the earlier match -- or beyond the budget, which changes nothing."""
    rng = np.random.default_rng(1950 + length)
    P = b'qRsTu'
    lines = []
    for at in range(0, min(66, length - 11)):
        for first in (b'QrStU', b'QRS#U', b'qr#tu', b'Q#T#', b'#RS#U') + ((b'QRTU', b'qr#STU') if kind is EDIT else ()):
            e = bytearray(filler(rng, length))
            e[at:at + len(first)], e[length - 5:] = first, P.swapcase() if at % 2 else P
            lines.append(bytes(e))
    r, ref, data = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, [P, P, P], [1, 2, 0])
        assert res.counts.tolist() == [len(lines)] * 3
    finally:
        r.close()


# ---- 13: load widths ---------------------------------------------------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_pattern_lengths_at_every_alignment(kind, k):
    """Pattern lengths k + 1 .. 17 and 23, 24, 25, each planted in another spelling at every alignment against the 8-byte
    word: within budget (one substitution in every piece but the last) and beyond it (one more, in the last piece)."""
    rng = np.random.default_rng(1960 + k)
    lines, patterns = [], []

    def add(body, lead):            # body in an entry of its own, at an offset of the chunk that is lead mod 8
        at = sum(len(x) + 1 for x in lines)
        lines.append(b'#' * ((lead - at) % 8) + body)

    for L in [n for n in list(range(1, 18)) + [23, 24, 25] if n > k]:
        P = WORD[:L]
        cut = near_pieces(P, k)
        ops = [off + len(piece) - 1 for off, piece in cut[:-1]]
        patterns.append(P)
        for lead in range(8):
            add(substituted(mangled(rng, P), ops) + filler(rng, int(rng.integers(0, 6))), lead)
            add(substituted(mangled(rng, P), ops + [L - 1]), lead)
    r, ref, data = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, patterns, k)
        assert (res.counts >= 8).all()
    finally:
        r.close()


# ---- 14, 15, 16: budgets, the relations of the contract, an edit beside a case flip -----------------------------------------

def test_mixed_budgets_and_the_three_relations():
    rng = np.random.default_rng(1970)
    lines = [mangled(rng, filler(rng, int(rng.integers(0, 30)))) for _ in range(300)]
    r, near_ref, data = one_chunk(NEAR, lines)
    edit_ref = EditIcaseRef([data])
    try:
        patterns = [b'a', b'aB', b'Abc', b'mnop', b'PON', b'zz', b'abcdEFGH', b'ponmlk', b'P', b'hgf']
        patterns += [lines[int(i)][1:int(rng.integers(3, 12))].swapcase() for i in rng.integers(0, len(lines), 24) if len(lines[int(i)]) >= 12]
        # k = 0 is the case-insensitive search, order included, for both kinds
        icase = r.search_icase_ids_batch(patterns)
        for kind, ref in ((NEAR, near_ref), (EDIT, edit_ref)):
            got = check(kind, r, ref, patterns, 0)
            assert np.array_equal(got.ids, icase.ids) and np.array_equal(got.counts, icase.counts) and got.ids.size > 300
            assert r.last_stats()['hits'] == sum(near_ref.piece_hits(p, 0) for p in patterns)
        ks = [min(int(rng.integers(0, 4)), len(p) - 1) for p in patterns]
        assert {0, 1, 2, 3} <= set(ks)
        near, edit = check(NEAR, r, near_ref, patterns, ks), check(EDIT, r, edit_ref, patterns, ks)
        exact_near, exact_edit = r.search_near_ids_batch(patterns, ks), r.search_near_ids_batch(patterns, ks, edits=True)
        again = r.search_near_ids_batch(patterns, ks, icase=False)
        assert np.array_equal(exact_near.ids, again.ids) and np.array_equal(exact_near.counts, again.counts)
        more_fold = more_edit = 0
        for p, kk, n, e, xn, xe in zip(patterns, ks, per_pattern(near), per_pattern(edit), per_pattern(exact_near), per_pattern(exact_edit)):
            assert set(xn.tolist()) <= set(n.tolist()) and set(xe.tolist()) <= set(e.tolist()) and set(n.tolist()) <= set(e.tolist()), (p, kk)
            more_fold += n.size > xn.size
            more_edit += e.size > n.size
        assert more_fold >= 10 and more_edit >= 5
        for k in range(4):          # every pattern of the mixed batch: what a batch of its own budget returns
            some = [i for i, kk in enumerate(ks) if kk == k]
            for kind, ref, mixed in ((NEAR, near_ref, near), (EDIT, edit_ref, edit)):
                alone = per_pattern(check(kind, r, ref, [patterns[i] for i in some], k))
                for i, ids in zip(some, alone):
                    assert np.array_equal(per_pattern(mixed)[i], ids), (patterns[i], k)
    finally:
        r.close()


@pytest.mark.parametrize('k', [1, 2, 3])
def test_an_edit_beside_a_case_flip(k):
    """Per piece in turn the fold-exact one: k edits -- an inserted, a deleted or a substituted byte -- right beside bytes in
    the other case, left of the piece, right of it or on both sides; and the same with k + 1.  The reference decides."""
    rng = np.random.default_rng(1980 + k)
    P = WORD[:11 + k]
    lines, planted = [], []
    for j, (off, piece) in enumerate(near_pieces(P, k)):
        left, right = list(range(0, off)), list(range(off + len(piece) + 1, len(P)))
        for side in ('left', 'right', 'both'):
            for op in ('ins', 'del', 'sub'):
                for e in (k, k + 1):
                    nl = {'left': e, 'right': 0, 'both': e // 2}[side]
                    if nl > len(left) or e - nl > len(right) or (side == 'both' and (nl == 0 or e - nl == 0)):
                        continue
                    at = rng.choice(left, nl, replace=False).tolist() + rng.choice(right, e - nl, replace=False).tolist()
                    planted.append(len(lines))
                    lines.append(filler(rng, int(rng.integers(0, 20))) + edited(P.swapcase(), [(op, int(i)) for i in at]) + filler(rng, int(rng.integers(0, 20))))
    lines += [filler(rng, int(rng.integers(0, 40))) for _ in range(20)]
    r, ref, data = one_chunk(EDIT, lines)
    try:
        got = set(check(EDIT, r, ref, [P], k).ids.tolist())
        assert got <= set(planted) and len(got) >= 3 * (k + 1) and len(set(planted) - got) >= 3, (len(got), len(planted))
        assert r.search_near_ids_batch([P], k, edits=True).ids.size == 0
    finally:
        r.close()


# ---- 17: placement and the interval routes ------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(1990)
    lines = [mangled(rng, filler(rng, int(rng.integers(0, 16)))) for _ in range(200)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    refs = {NEAR: NearIcaseRef.from_index(p), EDIT: EditIcaseRef.from_index(p)}
    patterns = []
    while len(patterns) < 90:
        ln = lines[int(rng.integers(0, len(lines)))]
        if len(ln) >= 9:
            at = int(rng.integers(0, len(ln) - 8))
            a = bytearray(ln[at:at + 9].swapcase())
            if rng.random() < 0.5:
                a[int(rng.integers(0, 9))] = ord('#')
            patterns.append(bytes(a))
    return p, refs, patterns


@KINDS
@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, kind, route, env):
    """90 patterns of 9 letters at k = 1: pieces of 4 and 5 letters, 16 + 32 spellings, more than 2 048 (query, chunk) pairs --
    the 16-lane interval search; the switches force the other two.  (One reference per kind, shared by the three.)"""
    p, refs, patterns = shape_index
    search_env(**env)
    r = pysubstringsearch.Reader(p)
    try:
        res = check(kind, r, refs[kind], patterns, 1, interval=R[route])
        assert res.ids.size >= 90 and (res.counts > 0).sum() > 60
    finally:
        r.close()


@KINDS
def test_placement(kind, tmp_path, search_env):
    rng = np.random.default_rng(2000)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else mangled(rng, filler(rng, int(rng.integers(0, 24)))) for i in range(1000)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 3000)
    ref = kind.ref_cls.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'abcd', b'head0', b'Head1', b'ead12', b'PONM', b'missing', b'HEAD 0', b'd012 ', b'MNopab', b'hed04', b'heead00']
    patterns += [ch.entry(0)[1:9].swapcase() for ch in ref.chunks if len(ch.entry(0)) >= 5]                    # at offset 0 of every chunk
    patterns += [lines[int(i)][1:8].swapcase() for i in rng.integers(0, len(lines), 12) if len(lines[int(i)]) >= 8]
    ks = [min(int(rng.integers(0, 3)), len(q) - 1) for q in patterns]
    # devices=[0, 0]: the merge is part-major inside a pattern, so the stated order is not compared there
    base = H.placement(kind, p, (patterns, ks), search_env, order_multi=False, ref=ref)
    assert base.ids.size > 100 and np.unique(base.ids >> np.uint64(32)).size >= 5


# ---- 18: empty inputs; errors; the conveniences ------------------------------------------------------------------------------

@KINDS
def test_an_empty_chunk_list_and_an_empty_batch(kind):
    edits = kind is EDIT
    r = device_reader([])
    try:
        ref = kind.ref_cls([])
        res = check(kind, r, ref, [b'Error', b'12', b'x\ny'], [1, 1, 2])
        assert res.ids.size == 0 and res.counts.tolist() == [0, 0, 0]
        assert check(kind, r, ref, [], 1).counts.size == 0
    finally:
        r.close()
    r, ref, data = one_chunk(kind, [b'Error', b'x'])
    try:
        res = check(kind, r, ref, [], 2)
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_near_batch_packed([], 1, edits=edits, icase=True).offsets.tolist() == [0] and r.count_near_bytes([], [], edits, icase=True) == []
        # a pattern that a newline voids: no hit is looked at, however often its seeds occur
        got = check(kind, r, ref, [b'R\nX', b'eR\nOr'], [1, 2])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
        assert check(kind, r, ref, [b'eRROR', b'X'], [1, 0]).counts.tolist() == [1, 1]
    finally:
        r.close()


def test_errors_and_conveniences(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    for e in ('Password', 'PASSW0RD!', 'my pasword', 'PassSword', 'pass-WORD', 'psswrd', 'drowssap', 'ÉTÉ court'):
        w.add_entry(e)
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert sorted(r.search_near('password', 1, icase=True)) == ['PASSW0RD!', 'Password'] and r.search_near('password', 1) == ['Password']
        assert sorted(r.search_near('password', k=1, edits=True, icase=True)) == ['PASSW0RD!', 'PassSword', 'Password', 'my pasword', 'pass-WORD']
        assert r.search_near('password', 0, icase=True) == r.search_icase('password') == ['Password']
        assert r.count_near('password', 1, icase=True) == 2 and r.count_near('password', 1, True, icase=True) == 5
        assert r.count_near('pass\nword', icase=True) == 0
        # only ASCII folds: `É` is two bytes that match only themselves
        assert r.search_near('été court', 0, icase=True) == [] and r.search_near('Été court', 2, icase=True) == ['ÉTÉ court']
        calls = (r.search_near_batch_packed, r.search_near_ids_batch, r.count_near_bytes)
        for edits in (False, True):
            for call in calls:
                with pytest.raises(ValueError, match='empty'):
                    call([b'ab', b''], 0, edits, icase=True)
                with pytest.raises(ValueError, match='budget of 3'):
                    call([b'abcd', b'abc'], 3, edits, icase=True)
                for k in (4, -1, [1, 4], [1]):
                    with pytest.raises(ValueError):
                        call([b'abcdef', b'abcdef'], k, edits, icase=True)
                for bad in (1, 'yes', None):
                    with pytest.raises(TypeError, match='icase'):
                        call([b'abcdef'], 1, edits, icase=bad)
            for call in (r.search_near, r.count_near):
                with pytest.raises(ValueError):
                    call('', edits=edits, icase=True)
                with pytest.raises(ValueError):
                    call('abc', 3, edits, icase=True)
                with pytest.raises(TypeError, match='icase'):
                    call('abcdef', 1, edits, icase=1)
        # through the C ABI with a reader: PSS_EINVAL with a message, *out and counts untouched; then a good batch
        h = r._handle()
        for edits in (0, 1):
            unit = 'edits' if edits else 'mismatches'
            for blob, offs, ks, what in ((b'abc', [0, 2, 2, 3], [0, 0, 0], 'pattern 1 is empty'), (b'abcdef', [0, 2, 4, 6], [1, 2, 1], 'pattern 1 has 2 bytes'),
                                         (b'abcdef', [0, 2, 4, 6], [1, 1, 4], 'pattern 2 has a budget of 4 ' + unit)):
                offs, ks = np.array(offs, dtype=np.uint64), np.array(ks, dtype=np.uint8)
                for fn in (_ffi.lib.pss_reader_search_near_icase_batch, _ffi.lib.pss_reader_search_near_icase_ids_batch):
                    out = ctypes.c_void_p()
                    assert fn(h, blob, offs.ctypes.data, 3, ks.ctypes.data, edits, ctypes.byref(out)) == _ffi.PSS_EINVAL
                    assert not out.value and what in _ffi.last_error()
                counts = np.full(4, 7, dtype=np.uint64)
                assert _ffi.lib.pss_reader_count_near_icase_batch(h, blob, offs.ctypes.data, 3, ks.ctypes.data, edits, counts.ctypes.data) == _ffi.PSS_EINVAL
                assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
            offs, ks = np.array([0, 8, 10], dtype=np.uint64), np.array([1, 0], dtype=np.uint8)
            out = ctypes.c_void_p()
            assert _ffi.lib.pss_reader_search_near_icase_batch(h, b'PASSWORDmy', offs.ctypes.data, 2, ks.ctypes.data, edits, ctypes.byref(out)) == _ffi.PSS_OK
            assert _ffi.lib.pss_result_num_entries(out) == (5 if edits else 2) + 1
            _ffi.lib.pss_result_free(out)
    finally:
        r.close()
