"""Any-of search (Reader.search_any_ids_batch / search_any_batch_packed / count_any_bytes, with and without icase=True, and
the str conveniences) against the brute force of tests/any_ref.py: an entry matches a set when one of the alternatives AS
GIVEN is in its true bytes.  Every set of every batch goes through the one check() of tests/search_harness.py, under the
two kinds tests/any_ref.py defines:
  * per set, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk by the alternative of the normalised set that stands at
    the entry's leftmost match, under fold then by the spelling of its seed, then in suffix-array order;
  * entry by entry, entries_by_id_packed(ids) is the packed text result, and every entry's text is the reference's;
  * `hits` is the sum of the exact occurrences of every query (any_ref.AnyRef.hits);
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), nothing else.
The cases follow DESIGN.md 4.22."""
import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import any_alternatives
from tests import search_harness as H
from tests.any_ref import ANY, ANY_ICASE, AnyIcaseRef, AnyRef
from tests.search_harness import device_reader, filler, make_index, per_row

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize('kind', [ANY, ANY_ICASE], ids=['exact', 'icase'])
# (no byte of the filler, under fold either; LONG is past the 8-byte register compare and past one 64-byte step with its entry)
LONG = b'QrStUvWxYz0123456789qRsTuVwXyZ9876543210QRST'
SHORT = b'#!'


def check(kind, r, ref, sets, **kw):
    return H.check(kind, r, ref, [list(s) for s in sets], **kw)


def one_chunk(kind, lines, closed=True):
    return H.one_chunk(kind.ref_cls, lines, closed)


def mangled(rng, b):
    """b with the case of each ASCII letter drawn anew."""
    return bytes(c ^ 0x20 if 0x61 <= (c | 0x20) <= 0x7a and rng.random() < 0.5 else c for c in b)


def spelt(kind, rng, b):
    return mangled(rng, b) if kind is ANY_ICASE else b


def ids_of(kind, ref, alts):
    return set(kind.want(ref, list(alts)).tolist())


# ---- one hit per entry ---------------------------------------------------------------------------------------------------------

@KINDS
def test_an_entry_that_holds_several_alternatives_several_times_comes_once(kind):
    rng = np.random.default_rng(2210)
    alts = [b'ERROR7', b'warn', b'Fatal42', b'Z']
    lines = []
    for i in range(240):
        body = [filler(rng, int(rng.integers(0, 12)))]
        for _ in range(int(rng.integers(0, 6))):
            body += [spelt(kind, rng, alts[int(rng.integers(0, len(alts)))]), filler(rng, int(rng.integers(0, 70 if i % 9 == 0 else 9)))]
        lines.append(b''.join(body))
    r, ref, _ = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, [alts, alts[:2], alts[2:]])
        several = sum(len(h) >= 2 for h in ref.holding(alts))
        assert several > 40 and res.counts[0] > 150
        # the same through the str conveniences
        texts = [a.decode() for a in alts]
        got = r.search_any(texts, icase=kind is ANY_ICASE)
        assert len(got) == r.count_any(texts, icase=kind is ANY_ICASE) == int(res.counts[0]) and len(set(got)) <= len(got)
    finally:
        r.close()


@KINDS
def test_overlapping_alternatives_keep_the_entry_at_the_left_one(kind):
    """`abc|bcd` on `abcd`: both stand, one byte apart; the entry comes once, under `abc` (the order says so)."""
    lines = [b'abcd', b'xabcdx', b'bcd', b'abc', b'ab', b'bcdabc', b'bcabcd', b'', b'abcabcd', b'cd abcd', b'aabbccdd']
    if kind is ANY_ICASE:
        lines += [b'ABcd', b'aBCD', b'xABCdx', b'BCDabc', b'abCD']
    r, ref, _ = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, [[b'abc', b'bcd'], [b'bcd', b'abc'], [b'bcd'], [b'abc']])
        first = per_row(res)[0].tolist()
        assert first.index(0) < first.index(2) and np.array_equal(per_row(res)[0], per_row(res)[1])       # `abcd` under abc, `bcd` under bcd
    finally:
        r.close()


# ---- the bound that changes: alternatives of several lengths ---------------------------------------------------------------------

@KINDS
@pytest.mark.parametrize('closed', [True, False], ids=['closed', 'unterminated'])
def test_a_long_alternative_that_starts_just_before_a_short_match(kind, closed):
    """The long alternative's first 1, 8 and 12 bytes right in front of the short one's match: at an entry's end inside the
    chunk, at the chunk's last byte (closed=False: no newline follows, then only the padding) and at the chunk's first byte.
    The scan for the long one must stop where it no longer fits into the entry."""
    rng = np.random.default_rng(2220)
    assert len(LONG) >= 40 and SHORT not in LONG
    tails = [LONG[:k] + SHORT for k in (1, 8, 12, len(LONG) - 1)]
    lines = [tails[0]]                                                      # the chunk's first byte
    for t in tails:
        for pad in (0, 1, 7, 8, 9, 55, 56, 57, 63, 64, 65, 120):
            lines.append(filler(rng, pad) + t)                              # at an entry's end
            lines.append(filler(rng, pad) + t + filler(rng, 3))
    lines += [LONG + SHORT, filler(rng, 5) + LONG + b' ' + SHORT, LONG[:20], LONG[20:] + SHORT, SHORT + LONG, LONG[1:] + SHORT, SHORT]
    lines.append(filler(rng, 61) + LONG[:8] + SHORT)                        # the chunk's last byte
    if kind is ANY_ICASE:
        lines = [mangled(rng, ln) if i % 2 else ln for i, ln in enumerate(lines[:-1])] + lines[-1:]
    r, ref, data = one_chunk(kind, lines, closed)
    try:
        assert data.startswith(LONG[:1] + SHORT) and data.endswith(SHORT + (b'\n' if closed else b''))
        res = check(kind, r, ref, [[LONG, SHORT], [SHORT, LONG], [LONG], [LONG, b'!']])
        assert res.counts[0] == len(lines) - 1 and res.counts[2] >= 3
    finally:
        r.close()
    # the same tails as the LAST entry of an unterminated chunk, one reader each: a match flush with n
    for t in tails[:3] + [LONG, SHORT]:
        r, ref, data = one_chunk(kind, [filler(rng, 40), t], closed)
        try:
            assert check(kind, r, ref, [[LONG, SHORT]]).counts.tolist() == [1]
        finally:
            r.close()


@KINDS
def test_alternatives_of_1_8_9_and_70_bytes(kind):
    rng = np.random.default_rng(2230)
    alts = [b'%', b'Qr5tUvWx', b'qR5TuVwXy'[::-1], bytes(rng.integers(0x51, 0x5b, 70, dtype=np.uint8))]
    assert [len(a) for a in alts] == [1, 8, 9, 70] and len(any_alternatives(alts, kind is ANY_ICASE)) == 4
    lines = []
    for a in alts:
        for pad in range(0, 18):
            lines.append(filler(rng, pad) + spelt(kind, rng, a) + filler(rng, int(rng.integers(0, 4))))
        lines.append(filler(rng, 70) + a[:-1])                              # all but the last byte
        lines.append(a[1:] + filler(rng, 3))
    lines += [filler(rng, 30) for _ in range(20)] + [alts[3] + alts[1] + alts[0], alts[0] * 3, alts[2][:-1] + alts[1]]
    r, ref, _ = one_chunk(kind, lines, closed=False)
    try:
        res = check(kind, r, ref, [alts, alts[1:], [alts[3]], [alts[0], alts[3]]])
        assert res.counts[0] >= 4 * 18 and res.counts[2] >= 18
    finally:
        r.close()


@KINDS
def test_an_alternative_that_ends_in_0x00_against_the_padding(kind):
    """The terms are followed by zero bytes on the device, the text too: `ab\\x00` is not in an unterminated chunk that ends
    in `ab`, and a term's zero padding is not part of its last alternative."""
    nine = b'QRSTUVWX\x00'
    lines = [b'ab\x00', b'x ab\x00 y', b'ab', b'QRSTUVWX\x00', b'QRSTUVWX', b'\x00', b'z\x00\x00', b'zz', b'xx ab']
    for closed in (True, False):
        r, ref, data = one_chunk(kind, lines, closed)
        try:
            res = check(kind, r, ref, [[b'ab\x00', nine], [nine], [b'zz\x00'], [b'\x00'], [b'ab\x00'], [b'b\x00', b'X\x00']])
            assert res.counts.tolist() == [3, 1, 0, 5, 2, 3]
        finally:
            r.close()


@KINDS
def test_bytes_from_0x80_on(kind):
    lines = [b'\xc9t\xe9', b'\xe9T\xe9', b'\xe9t\xe9 court', b'\xc9T\xc9', b'\xff\xfe\xff', b'\x80\x81', b'ete', b'\xe9', b'\xff\xff\xfe\xff\x80']
    r, ref, _ = one_chunk(kind, lines, closed=False)
    try:
        res = check(kind, r, ref, [[b'\xe9t\xe9', b'\xff\xfe'], [b'\xc9'], [b'\x80', b'\xe9T'], [b'\xfe\xff\x80', b'\xc9t']])
        assert res.counts.tolist() == ([4, 2, 4, 3] if kind is ANY_ICASE else [3, 2, 3, 2])       # (`T` folds, `\xc9` does not)
    finally:
        r.close()


# ---- full sets ---------------------------------------------------------------------------------------------------------------------

def distinct(n):
    return [bytes([0x30 + i // 10, 0x71 + i % 10]) for i in range(n)]                  # `0q` .. `6z`: no filler byte


@KINDS
def test_a_set_at_its_cap(kind):
    rng = np.random.default_rng(2240)
    n = 32 if kind is ANY_ICASE else 64
    alts = distinct(n)
    lines = []
    for i in range(300):
        parts = [filler(rng, int(rng.integers(0, 10)))]
        for _ in range(int(rng.integers(0, 4))):
            parts += [spelt(kind, rng, distinct(70)[int(rng.integers(0, 70))]), filler(rng, int(rng.integers(0, 10)))]
        lines.append(b''.join(parts))
    r, ref, _ = one_chunk(kind, lines)
    try:
        assert len(any_alternatives(alts, kind is ANY_ICASE)) == n
        res = check(kind, r, ref, [alts, alts[::-1], alts[:n // 2], alts + alts[:5] + [alts[0] + b'x', b'y\n' + alts[1]]])
        assert 100 < res.counts[0] < 300 and res.counts[3] == res.counts[0]
        with pytest.raises(ValueError, match='after normalisation'):
            r.search_any_ids_batch([distinct(n + 1)], icase=kind is ANY_ICASE)
    finally:
        r.close()


# ---- under fold ------------------------------------------------------------------------------------------------------------------

def test_mixed_spellings_of_two_alternatives_in_one_entry():
    rng = np.random.default_rng(2250)
    alts = [b'Error', b'WARNING']
    lines = [b' '.join(mangled(rng, alts[int(rng.integers(0, 2))]) for _ in range(int(rng.integers(1, 6)))) for _ in range(200)]
    lines += [b'error', b'ERROR', b'warning', b'WARNING', b'erro', b'arning', b'eRRoRwARNiNG', b'wARNiNGeRRoR']
    r, ref, _ = one_chunk(ANY_ICASE, lines)
    try:
        res = check(ANY_ICASE, r, ref, [alts])
        assert res.counts.tolist() == [len(lines) - 2]
        exact = r.search_any_ids_batch([alts])
        assert set(exact.ids.tolist()) < set(res.ids.tolist())
    finally:
        r.close()


@pytest.mark.parametrize('letters', [1, 6, None])
def test_seed_letters_and_two_alternatives_with_the_same_seed(letters, search_env):
    """`ab1234` and `cb1234` at one letter: both are looked up through `b1234` / `B1234`, so every occurrence of the seed is
    a hit of both queries' intervals -- the pair's sum is twice the seed's occurrences, and `hits` says so."""
    rng = np.random.default_rng(2260)
    search_env(PSS_ICASE_SEED_LETTERS=letters)
    alts = [b'ab1234', b'cb1234']
    lines = [b'ab1234', b'CB1234', b'xb1234', b'ab1234cb1234', b'cB1234 Ab1234', b'b1234', b'aab1234', b'abcb1234', b'B1234B1234cb1234']
    lines += [mangled(rng, filler(rng, int(rng.integers(0, 20)))) for _ in range(100)]
    r, ref, _ = one_chunk(ANY_ICASE, lines, closed=False)
    try:
        ref.letters = any_ref_letters = 5 if letters is None else letters
        asked = any_alternatives(alts, True)
        assert asked == any_alternatives(alts, True, any_ref_letters)
        assert (asked[0][2] == asked[1][2] == b'b1234') == (letters == 1)
        words = [b'abcdefgh', b'ponmlkji', b'Hgfedcba12']
        res = check(ANY_ICASE, r, ref, [alts, words, alts + words])
        assert res.counts[0] == 7
        if letters == 1:
            assert r.count_any_bytes([alts], icase=True) == [7] and r.last_stats()['hits'] == 2 * sum(ln.lower().count(b'b1234') for ln in lines)
    finally:
        r.close()
        search_env(PSS_ICASE_SEED_LETTERS=None)


# ---- void sets, empty inputs, shared alternatives -----------------------------------------------------------------------------------

@KINDS
def test_a_set_voided_by_newlines_beside_a_live_one(kind):
    r, ref, data = one_chunk(kind, [b'Error here', b'x', b'or', b'Err', b'here'])
    try:
        res = check(kind, r, ref, [[b'r\nx', b'\n'], [b'Err', b'x\nor'], [b'here\nx\nor\nErr'], [b'x']])
        assert res.counts.tolist() == [0, 2, 0, 1]
        # every set void: the batch has no query at all and is answered as an empty batch is -- zero counts, nothing launched
        icase = kind is ANY_ICASE
        void = [[b'\n'], [b'e\nx']]
        res = r.search_any_ids_batch(void, icase=icase)
        assert res.ids.size == 0 and res.counts.tolist() == [0, 0] and r.last_stats()['hits'] == 0 and r.last_stats()['queries'] == 2
        assert r.count_any_bytes(void, icase=icase) == [0, 0] and r.search_any_batch_packed(void, icase=icase).offsets.tolist() == [0]
    finally:
        r.close()


@KINDS
def test_an_empty_batch_and_a_reader_without_chunks(kind):
    icase = kind is ANY_ICASE
    r = device_reader([])
    try:
        ref = kind.ref_cls([])
        res = check(kind, r, ref, [[b'Error', b'12'], [b'x\ny']])
        assert res.ids.size == 0 and res.counts.tolist() == [0, 0]
        assert check(kind, r, ref, []).counts.size == 0
    finally:
        r.close()
    r, ref, _ = one_chunk(kind, [b'Error', b'x'])
    try:
        res = check(kind, r, ref, [])
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_any_batch_packed([], icase=icase).offsets.tolist() == [0] and r.count_any_bytes([], icase=icase) == []
        assert check(kind, r, ref, [[b'Error', b'X']]).counts.tolist() == [1 + icase]
    finally:
        r.close()


@KINDS
def test_two_sets_that_share_alternatives(kind):
    rng = np.random.default_rng(2270)
    words = [b'Qrst', b'UV12', b'wxyZ9', b'%%', b'Q']
    lines = [b''.join([filler(rng, int(rng.integers(0, 9))), spelt(kind, rng, words[int(rng.integers(0, 5))]), filler(rng, int(rng.integers(0, 9)))])
             if rng.random() < 0.6 else filler(rng, int(rng.integers(0, 15))) for _ in range(300)]
    r, ref, _ = one_chunk(kind, lines)
    try:
        res = check(kind, r, ref, [words[:3], words[1:4], words[2:], words[:1], words[:3]])
        rows = per_row(res)
        assert np.array_equal(rows[0], rows[4]) and rows[0].size > 40
    finally:
        r.close()


# ---- the identities ----------------------------------------------------------------------------------------------------------------

def identity_text():
    rng = np.random.default_rng(2280)
    lines = [mangled(rng, filler(rng, int(rng.integers(0, 40)))) for _ in range(400)] + [b'Password', b'passWORD password', b'PASSWORD']
    order = rng.permutation(len(lines))
    lines = [lines[int(i)] for i in order]
    cut = len(lines) // 2
    return [b'\n'.join(lines[:cut]) + b'\n', b'\n'.join(lines[cut:])]


PATTERNS = [b'a', b'ab', b'abc', b'p', b'Password', b'password', b'ssw', b'mnop', b'abcdefghi', b'missing', b'B', b'ponm', b'Ab']


def test_a_set_of_one_alternative_is_the_plain_search():
    chunks = identity_text()
    r = device_reader(chunks)
    try:
        assert r.result_order == 'text'
        plain = r.search_ids_batch(PATTERNS)
        one = check(ANY, r, AnyRef(chunks), [[p] for p in PATTERNS])
        assert np.array_equal(one.ids, plain.ids) and np.array_equal(one.counts, plain.counts) and plain.ids.size > 300
    finally:
        r.close()


def test_a_set_of_one_alternative_under_fold_is_the_case_insensitive_search():
    chunks = identity_text()
    r = device_reader(chunks)
    try:
        folded = r.search_icase_ids_batch(PATTERNS)
        one = check(ANY_ICASE, r, AnyIcaseRef(chunks), [[p] for p in PATTERNS])
        assert np.array_equal(one.ids, folded.ids) and np.array_equal(one.counts, folded.counts) and folded.ids.size > 600
    finally:
        r.close()


def test_a_row_is_the_union_of_its_alternatives_rows():
    chunks = identity_text()
    rng = np.random.default_rng(2290)
    sets = [[PATTERNS[int(i)] for i in rng.choice(len(PATTERNS), int(rng.integers(2, 7)), replace=False)] for _ in range(12)]
    r = device_reader(chunks)
    try:
        got = per_row(check(ANY, r, AnyRef(chunks), sets))
        for row, alts in zip(got, sets):
            union = np.unique(np.concatenate(per_row(r.search_ids_batch(alts))))
            assert np.array_equal(np.sort(row), union)
        got = per_row(check(ANY_ICASE, r, AnyIcaseRef(chunks), sets))
        for row, alts in zip(got, sets):
            union = np.unique(np.concatenate(per_row(r.search_icase_ids_batch(alts))))
            assert np.array_equal(np.sort(row), union)
    finally:
        r.close()


# ---- the harness scenarios -----------------------------------------------------------------------------------------------------------

@KINDS
def test_layout_edges(kind):
    """63 / 64 / 65 sets whose alternatives' bytes add up to 31 / 32 / 33 modulo 64, on one chunk and on three."""
    H.layout_edges(kind, lambda groups: [[a, b] for a, b, _ in groups])


@KINDS
def test_placement(kind, tmp_path, search_env):
    rng = np.random.default_rng(2300)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else mangled(rng, filler(rng, int(rng.integers(0, 24)))) for i in range(1000)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 3000)
    ref = kind.ref_cls.from_index(p)
    assert len(ref.chunks) >= 5
    sets = [[b'abcd', b'head0'], [b'Head1', b'ead12', b'PONM'], [b'missing', b'absent'], [b'HEAD 0', b'd012 ', b'MNopab'], [b'a\nb', b'HEAD'],
            [b'e', b'P', b'HEAD'], [b'ab', b'CD']]                      # (hundreds of entries in either form)
    sets += [[ch.entry(0)[:8], ch.entry(0)[1:5]] for ch in ref.chunks if len(ch.entry(0)) >= 8]                    # at offset 0 of every chunk
    sets += [[lines[int(i)][1:8] for i in rng.integers(0, len(lines), 4) if len(lines[int(i)]) >= 8] + [b'HEAD9'] for _ in range(6)]
    # devices=[0, 0]: the merge is part-major inside a set, so the stated order is not compared there
    base = H.placement(kind, p, sets, search_env, order_multi=False, ref=ref)
    assert base.ids.size > 100 and np.unique(base.ids >> np.uint64(32)).size >= 5
