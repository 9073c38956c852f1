"""Case-insensitive search (Reader.search_icase_ids_batch / search_icase_batch_packed / count_icase_bytes and the str
conveniences) against the brute-force reference of tests/icase_ref.py.  Every pattern of every batch goes through one
check():
  * per pattern, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * the ids come in the stated order: chunk-major, inside a chunk the suffix-array order of the seed's occurrence inside
    each entry's leftmost folded match (the reference sorts the suffixes themselves);
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result, and every entry's text is the
    reference's for its id;
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), none of ANCHORED, MID, SMALL_*, RESIDENT,
    SA_ORDER.
The cases: what folds and what does not; the verify step outside the seed (near misses on both sides, a seed at the
chunk's first bytes, a match that would end past n); the leftward scan for an earlier folded occurrence (same word, same
64-byte step, one and two steps back, overlapping, at every (lane, byte), entry prefixes around the load widths); chunk
edges; the seed-letters switch and the `hits` it decides; letterless patterns; more candidates than the mid pipeline
holds; the three interval routes; placement; errors and conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, icase_variants
from tests import search_harness as H
from tests.icase_ref import IcaseRef, folded_occurrences
from tests.icase_texts import PAIRS_0X20, mangle, mixed_case_lines
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu


def spellings(word):
    return icase_variants(word, 6)[1] if len(word) <= 6 else None


def check(r, ref, patterns, **kw):
    """patterns on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.ICASE, r, ref, list(patterns), **kw)


def one_chunk(lines, closed=True):
    return H.one_chunk(IcaseRef, lines, closed)


# ---- 1. meaning ---------------------------------------------------------------------------------------------------

def test_meaning():
    rng = np.random.default_rng(131)
    lines = [b'Error', b'ERROR', b'error', b'eRrOr', b'terror', b'err or', b'ERR0R', b'erro', b'rror',
             b'error .. ERROR', b'ERROR .. error', b'Error error ERROR eRROR', b'x ERROR y Error z', b'']
    lines += [filler(rng, int(rng.integers(0, 30))) for _ in range(200)]
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    r, ref, data = one_chunk(lines)
    try:
        every = icase_variants(b'error', 5)[1]
        assert len(every) == 32 and b'eRrOr' in every
        res = per_pattern(check(r, ref, every))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        want = sorted([b'Error', b'ERROR', b'error', b'eRrOr', b'terror', b'error .. ERROR', b'ERROR .. error', b'Error error ERROR eRROR',
                       b'x ERROR y Error z'])
        for got in res:
            assert texts(got) == want and np.array_equal(got, res[0])           # every spelling: the same ids in the same order
        # `ERROR` sorts in front of `error`, but an entry is kept at its LEFTMOST match: the mirror comes first
        ids = res[0].tolist()
        at = {t: ids.index(i) for t, i in zip(r.entries_by_id(ids), ids)}
        assert at[b'ERROR .. error'] < at[b'error .. ERROR']
        assert r.last_stats()['hits'] == 32 * folded_occurrences(data, b'error')  # (32 patterns, the same candidates each)
        res = per_pattern(check(r, ref, [b'ERR', b'rOR', b'r', b'err or', b'ERR OR', b'Rr0', b'error .. error', b'z eRROR', b'nope', b'.. '
                                         ]))
        assert texts(res[3]) == texts(res[4]) == [b'err or'] and texts(res[5]) == [b'ERR0R'] and res[8].size == 0
        assert texts(res[6]) == [b'ERROR .. error', b'error .. ERROR'] and texts(res[7]) == []
    finally:
        r.close()


# ---- 2. what does not fold ----------------------------------------------------------------------------------------------

def test_bytes_that_differ_by_0x20_and_are_no_letters():
    lines = []
    for lo, hi in PAIRS_0X20:
        lines += [b'x' + lo + b'y', b'X' + hi + b'Y', lo, hi, b'pad ' + lo + lo + hi + b' pad', lo * 9 + b'Q', hi * 9 + b'q']
    lines += [b'az', b'AZ', b'@Z[', b'`z{', b'a' * 8 + b'@' * 8, b'A' * 8 + b'`' * 8]
    r, ref, data = one_chunk(lines)
    try:
        patterns = []
        for lo, hi in PAIRS_0X20:
            patterns += [lo, hi, b'x' + lo + b'Y', b'x' + hi + b'Y', lo + lo + hi, hi + hi + lo, lo * 9 + b'q', hi * 9 + b'Q']
        patterns += [b'az', b'@z[', b'`Z{', b'AAAAAAAA@@@@@@@@', b'aaaaaaaa````````', b'@', b'z']
        res = per_pattern(check(r, ref, patterns))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        for k, (lo, hi) in enumerate(PAIRS_0X20):
            a, b, xa, xb, aab, bba, a9, b9 = res[8 * k:8 * k + 8]
            assert lo in texts(a) and hi not in texts(a) and hi in texts(b) and lo not in texts(b), (lo, hi)
            assert texts(xa) == [b'x' + lo + b'y'] and texts(xb) == [b'X' + hi + b'Y'], (lo, hi)
            assert texts(aab) == [b'pad ' + lo + lo + hi + b' pad'] and bba.size == 0
            assert texts(a9) == [lo * 9 + b'Q'] and texts(b9) == [hi * 9 + b'q']
    finally:
        r.close()


def test_zero_in_a_pattern_does_not_match_the_padding():
    texts = [b'xa\x00y\nbA', b'A', b'a\x00', b'\x00a\nA\x00\n\x00']
    r, ref = device_reader(texts), IcaseRef(texts)
    try:
        res = per_pattern(check(r, ref, [b'a\x00', b'A\x00', b'a', b'a\x00\x00', b'A\x00\x00\x00\x00\x00\x00\x00\x00', b'\x00', b'\x00a']))
        assert res[0].tolist() == res[1].tolist() == [0, 2 << 32, (3 << 32) | 1]
        assert sorted(res[2].tolist()) == [0, 1, 1 << 32, 2 << 32, 3 << 32, (3 << 32) | 1]
        assert res[3].size == 0 and res[4].size == 0
    finally:
        r.close()


# ---- 3. the verify step: the bytes outside the seed ---------------------------------------------------------------------

WORD = b'qrstuvwxyz' * 2
VERIFY_PATTERNS = [WORD[:n] for n in range(7, 21)] + [b'qrs_tuvwxy12345678', b'12qrstuv_wxyz', b'qr=st=uv=wx=yz=qr', b'zyxwvutsrq9']


def test_the_whole_pattern_is_verified_around_the_seed():
    """Per pattern: the pattern itself in three spellings, the same with the case flipped OUTSIDE the seed only (matches),
    and two near misses -- the byte left of the seed and the byte right of it changed (the seed still hits).  The filler
    lacks the patterns' letters under either case."""
    rng = np.random.default_rng(132)
    lines, expect = [], {}
    offs = set()
    for p in VERIFY_PATTERNS:
        so, var = icase_variants(p)
        sl = len(var[0])
        offs.add(so)
        assert sl < len(p)
        outside = bytes(b ^ 0x20 if (i < so or i >= so + sl) and chr(b).isalpha() else b for i, b in enumerate(p))
        good = [p, p.upper(), mangle(rng, p), outside, mangle(rng, outside)]
        bad = []
        if so > 0:
            bad.append(p[:so - 1] + b'#' + p[so:])
        if so + sl < len(p):
            bad.append(p[:so + sl] + b'#' + p[so + sl + 1:])
        bad.append(p[:-1])
        expect[p] = []
        for body, ok in [(g, True) for g in good] + [(b, False) for b in bad]:
            e = filler(rng, int(rng.integers(0, 20))) + body + filler(rng, int(rng.integers(0, 20)))
            if ok:
                expect[p].append(len(lines))
            lines.append(e)
    assert 0 in offs and len(offs) >= 3          # seeds at the pattern's start and inside it
    r, ref, data = one_chunk(lines)
    try:
        res = per_pattern(check(r, ref, VERIFY_PATTERNS))
        for p, got in zip(VERIFY_PATTERNS, res):
            # (a longer WORD prefix holds the shorter ones: at least the planted entries)
            assert set(expect[p]) <= set(got.tolist()) and got.size >= 5, p
        assert sorted(res[-1].tolist()) == expect[VERIFY_PATTERNS[-1]]
        assert r.last_stats()['hits'] > r.last_stats()['entries']              # the near misses were candidates
    finally:
        r.close()


def test_a_seed_hit_whose_match_would_leave_the_chunk():
    """Left: the seed's bytes open the chunk and the pattern's seed sits seed_off > 0 bytes in, so the match would start
    before the text.  Right: a pattern of more than 128 bytes whose seed hits near the end of an unterminated chunk, so
    the match would end past n -- and past the readable slack behind it.  Both are rejected before anything is read."""
    p_left = b'qrs_tuvwxy12345678'
    so, var = icase_variants(p_left)
    assert so == 5 and var[-1] == b'uvwxy12345678'
    p_right = b'qrstu' + b'0123456789' * 13 + b'vwxyzq'
    so_r, var_r = icase_variants(p_right)
    assert len(p_right) == 141 and so_r == 0 and len(var_r[0]) == 135
    p_mid = b'zz' + b'qrstu' + b'0123456789' * 13 + b'vwxyzq'            # the same with two bytes in front of the seed
    assert icase_variants(p_mid)[0] == 2
    texts = [p_left[so:].upper() + b' opens the chunk\nab ' + mangle(np.random.default_rng(1), p_left) + b'\nlast ' + p_right[:138],
             p_right[:135],                              # the whole chunk is the seed
             b'_' + p_mid[2:] + b'\n' + p_mid[1:] + b'\n' + p_mid.upper(),      # one byte short in front, twice; then the match ends at n
             p_left[so:]]
    r, ref = device_reader(texts), IcaseRef(texts)
    try:
        res = per_pattern(check(r, ref, [p_left, p_right, p_mid, p_left[so:], p_right[:135]]))
        assert res[0].tolist() == [1] and sorted(res[1].tolist()) == [2 << 32, (2 << 32) | 1, (2 << 32) | 2] and res[2].tolist() == [(2 << 32) | 2]
        assert sorted(res[3].tolist()) == [0, 1, 3 << 32] and sorted(res[4].tolist()) == [2, 1 << 32, 2 << 32, (2 << 32) | 1, (2 << 32) | 2]
        st = r.last_stats()
        assert st['hits'] > st['entries']
    finally:
        r.close()


# ---- 4. the leftward scan: an earlier folded occurrence ------------------------------------------------------------------

SCAN_PATTERNS = (b'QR7', b'qrstuvwxyz12', b'q')
GEOMS = {'word': (0, 4), 'word7': (1, 7), 'next_word': (7, 8), 'step': (3, 40), 'one_step_back': (3, 70), 'two_steps_back': (3, 140),
         'far': (60, 700)}


def test_an_earlier_folded_occurrence_drops_the_hit():
    """The pattern twice in an entry, in two spellings whose intervals lie apart (the upper-case one sorts first and
    stands to the RIGHT): the entry comes once, for its leftmost match.  Beside each such entry, one whose earlier
    occurrence is a near miss -- the last byte changed, so the first bytes match in registers -- which must be kept.
    Every geometry with the entry shifted by 0 .. 3 bytes against the 8-byte grid of the text.
    The last four entries and the last three patterns are the ends of the scanned range under fold: a range of ONE start
    position whose byte is a candidate and no match (decided in registers for `aB`, by the long compare for
    `aaaaaaaab`), and an earlier match that starts in the last, partial word of the range and is found by the long
    compare (ten `a` in twelve `A`: the matches at 7 and 8 stand in front of the one at 9)."""
    rng = np.random.default_rng(133)
    lines = []
    for P in SCAN_PATTERNS:
        miss = P[:-1].lower() + b'#' if len(P) > 1 else b'#'
        for name, (a1, a2) in GEOMS.items():
            if a1 + len(P) > a2:
                continue
            for lead in range(4):
                for first in (P.lower(), miss):
                    e = bytearray(filler(rng, a2 + len(P) + int(rng.integers(0, 12))))
                    e[a1:a1 + len(P)], e[a2:a2 + len(P)] = first, P.upper()
                    lines += [b'#' * lead, bytes(e)]
    lines += [b'xAaAx', b'AaA', b'aA', b'xaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAaAx', b'Qq', b'qQ', b'QQQQQQQQQq', b'qqqqqqqqqqQ']
    lines += [b'AaB', b'aAb', b'AaaaaaaaaB', b'xxxxxxxAAAAAAAAAAAA']
    r, ref, data = one_chunk(lines)
    try:
        res = per_pattern(check(r, ref, list(SCAN_PATTERNS) + [b'aa', b'AA', b'aA', b'aaa', b'qq', b'QQ', b'aB', b'aaaaaaaab', b'AAAAAaaaaa']))
        assert res[0].size == 2 * 4 * 6 and res[1].size == 2 * 4 * 4           # (the geometries each pattern's length fits)
        assert sorted(r.entries_by_id(res[3])) == sorted(r.entries_by_id(res[5])) == sorted([x for x in lines if b'aa' in x.lower()])
        assert {b'xAaAx', b'AaA', b'aA'} <= set(r.entries_by_id(res[3])) and {b'Qq', b'qQ', b'QQQQQQQQQq'} <= set(r.entries_by_id(res[7]))
        assert r.last_stats()['hits'] > r.last_stats()['entries'] + 2 * 4 * 10  # the later occurrences were candidates, and dropped
    finally:
        r.close()


def test_every_lane_and_byte_of_the_first_step():
    """An earlier occurrence at every position 0 .. 65 in front of a later one at 80: dropped wherever it stands; and a
    near miss at the same positions: kept."""
    rng = np.random.default_rng(134)
    lines = []
    for at in range(0, 66):
        for first in (b'qr7', b'qr#', b'q#7'):
            e = bytearray(filler(rng, 90))
            e[at:at + 3], e[80:83] = first, b'QR7'
            lines.append(bytes(e))
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [b'Qr7', b'qR'])
        assert res.counts.tolist() == [198, 198]
        assert r.last_stats()['hits'] == (198 + 66) + (198 + 132)              # every occurrence of the two seeds
    finally:
        r.close()


def test_entry_prefixes_around_the_load_widths():
    rng = np.random.default_rng(135)
    lines = []
    for lead in range(4):
        for k in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300):
            for body in (b'Qr7', b'qRsTuVwXyZ12'):
                lines += [b'#' * lead, filler(rng, k) + body + filler(rng, int(rng.integers(0, 9))), filler(rng, k) + body[:-1] + b'#']
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, [b'qr7', b'QRSTUVWXYZ12', b'qrstuvwxyz1'])
        assert res.counts.tolist() == [60, 60, 120]
    finally:
        r.close()


# ---- 5. chunk edges ---------------------------------------------------------------------------------------------------

def test_chunk_edges_handed_over_on_the_device():
    texts = [b'ONLYONE x\n',                                   # 0: a one-entry chunk
             b'Error first\n\n\nab\nmid x\nx last ERRor',        # 1: the entry at offset 0, empty entries, no closing newline
             b'noEND',                                         # 2: the whole chunk is one unterminated entry
             b'\n', b'x', b'X\n',                              # 3, 4, 5
             b'HEL\nLO x\nhello']                              # 6
    ref = IcaseRef(texts)
    r = device_reader(texts)
    try:
        patterns = [b'error', b'ERROR FIRST', b'rror f', b'onlyone X', b'e x', b'onlyone x ', b'MID X', b'AB', b'b',
                    # the unterminated last entry: the last byte takes part, and a match may end exactly at n
                    b'error', b'RROR', b'last error', b'rorx', b'NOEND', b'noend', b'oen', b'end', b'noendx', b'D', b'R', b'x',
                    b'hel\nlo', b'HELLO', b'lo X', b'l\n', b'\n']
        res = per_pattern(check(r, ref, patterns))
        at = {g: i for i, g in enumerate(patterns)}
        assert sorted(res[at[b'error']].tolist()) == [1 << 32, (1 << 32) | 5] and res[at[b'ERROR FIRST']].tolist() == [1 << 32]
        assert res[at[b'onlyone X']].tolist() == [0] and res[at[b'onlyone x ']].size == 0 and res[at[b'e x']].tolist() == [0]
        assert res[at[b'last error']].tolist() == [(1 << 32) | 5] and res[at[b'RROR']].size == 2 and res[at[b'rorx']].size == 0
        assert res[at[b'NOEND']].tolist() == res[at[b'noend']].tolist() == res[at[b'end']].tolist() == [2 << 32] and sorted(res[at[b'D']].tolist()) == [(1 << 32) | 4, 2 << 32]
        assert res[at[b'noendx']].size == 0 and res[at[b'oen']].tolist() == [2 << 32]
        assert r.entries_by_id([(1 << 32) | 5, 2 << 32]) == [b'x last ERRo', b'noEN']         # handed out without the last byte, matched with it
        assert sorted(res[at[b'x']].tolist()) == [0, (1 << 32) | 4, (1 << 32) | 5, 4 << 32, 5 << 32, (6 << 32) | 1]
        for g in (b'hel\nlo', b'l\n', b'\n'):
            assert res[at[g]].size == 0, g
        assert res[at[b'HELLO']].tolist() == [(6 << 32) | 2] and res[at[b'lo X']].tolist() == [(6 << 32) | 1]
        # a pattern that a newline voids: no hit is looked at, however often its seed occurs
        got = check(r, ref, [b'x\n', b'\nx', b'e\nx'])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
        assert r.count_icase_bytes([b'x\n']) == [0] and r.last_stats()['hits'] == 0
    finally:
        r.close()


def test_an_empty_chunk_list_and_an_empty_batch():
    r = device_reader([])
    try:
        ref = IcaseRef([])
        assert r.num_chunks == 0
        res = check(r, ref, [b'error', b'12', b'x\n'])
        assert res.ids.size == 0 and res.counts.tolist() == [0, 0, 0]
        res = check(r, ref, [])
        assert res.ids.size == 0 and res.counts.size == 0
    finally:
        r.close()
    r, ref, data = one_chunk([b'Error', b'x'])
    try:
        res = check(r, ref, [])
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_icase_batch_packed([]).offsets.tolist() == [0] and r.count_icase_bytes([]) == []
    finally:
        r.close()


def test_three_chunks_through_max_chunk_len(tmp_path):
    rng = np.random.default_rng(136)
    lines = mixed_case_lines(rng, 600)
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'three', data, 3000)
    ref = IcaseRef.from_index(p)
    assert 3 <= len(ref.chunks) <= 8
    r = pysubstringsearch.Reader(p)
    try:
        patterns = [b'ab', b'AB', b'abc', b'p', b'NOP', b'mnop', b'zz'] + [ch.entry(0) for ch in ref.chunks if ch.entry(0)]
        patterns += [lines[int(i)][2:9].swapcase() for i in rng.integers(0, len(lines), 20) if len(lines[int(i)]) >= 9]
        res = check(r, ref, patterns)
        chunk_of = (res.ids >> np.uint64(32)).astype(np.int64)
        group_of = np.repeat(np.arange(len(patterns)), res.counts.astype(np.int64))
        assert (np.diff(chunk_of)[np.diff(group_of) == 0] >= 0).all() and np.unique(chunk_of).size >= 3      # chunk-major inside a pattern
    finally:
        r.close()


# ---- 6. the seed-letters switch ---------------------------------------------------------------------------------------

def test_every_seed_length_gives_the_same_ids_in_the_same_order(search_env):
    """The order inside a (pattern, chunk) pair is the suffix order at the seed's occurrence, so it depends on the seed's
    OFFSET in the pattern and on nothing else of the seed.  The batch mixes patterns whose seed starts at the same offset
    under every F (letters only, no letter at all, non-letters in front) with patterns whose seed offset moves with F but
    which match one entry: identical ids in identical order under every F."""
    rng = np.random.default_rng(137)
    lines = mixed_case_lines(rng, 400, 4, 30)
    lines += [b'USER_ID=12345678', b'Abcdefgh here', b'x ABCDEFGH', b'12 34', b'abcdefg', b'ab', b'AB cd', b'abcdeF', b'ABCDEf', b'gh']
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    r, ref, data = one_chunk(lines)
    moving = [b'user_id=12345678', b'x abcdefgh', b'h HERE']
    fixed = [b'abcdefgh', b'ab', b'abc', b'ABCD', b'abcde', b'abcdef', b'abcdefg', b'mnop', b'12', b' ', b'12 34', b'=1234', b'12 ab', b'ponm', b'p']
    try:
        assert len({icase_variants(moving[0], F)[0] for F in range(1, 7)}) > 1
        for p in fixed:
            assert {icase_variants(p, F)[0] for F in range(1, 7)} == {0}
        for p in moving:
            assert ref.search_icase_ids(p).size == 1
        base = None
        for F in (5, 1, 2, 3, 4, 6):
            search_env(PSS_ICASE_SEED_LETTERS=F)
            got = check(r, ref, fixed + moving)
            base = got if base is None else base
            assert np.array_equal(got.ids, base.ids) and np.array_equal(got.counts, base.counts), F
        assert base.ids.size > 100
        # hits are the occurrences of that F's seed window under fold: more of them than of the pattern
        pat = b'abcdefgh'
        for F in (2, 6):
            search_env(PSS_ICASE_SEED_LETTERS=F)
            so, var = icase_variants(pat)
            assert (so, len(var), len(var[0])) == (0, 1 << F, F)
            want = ref.seed_hits(pat[:F])
            assert want > folded_occurrences(data, pat) == 2
            for call in (r.search_icase_ids_batch, r.search_icase_batch_packed, r.count_icase_bytes):
                call([pat])
                st = r.last_stats()
                assert st['hits'] == want and st['entries'] == 2 and st['queries'] == 1, (F, call.__name__)
    finally:
        r.close()


# ---- 7. letterless patterns ---------------------------------------------------------------------------------------------

def test_letterless_patterns_are_the_plain_search():
    rng = np.random.default_rng(138)
    abc = np.frombuffer(b'0123 _-=a', np.uint8)
    lines = [bytes(abc[rng.integers(0, len(abc), int(rng.integers(0, 20)))]) for _ in range(500)]
    r, ref, data = one_chunk(lines)
    try:
        patterns = [b'1', b'12', b'0 ', b'_-', b'=', b'123', b'3210', b' ', b'99', b'0123 _-=']
        for p in patterns:
            assert icase_variants(p) == (0, [p])
        got, plain = check(r, ref, patterns), r.search_ids_batch(patterns)
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts) and got.ids.size > 500
    finally:
        r.close()


# ---- 8. more candidates than the mid pipeline's 65 536 and than one scan workgroup; the interval routes -----------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    """100 000 entries of ten bytes, each with the seed of `qrstuvw` in some spelling and one of four tails, of which two
    complete the pattern under fold."""
    rng = np.random.default_rng(139)
    k = 100_000
    raw = np.empty((k, 10), dtype=np.uint8)
    raw[:, 0], raw[:, 8], raw[:, 9] = ord('a'), ord('b'), 0x0A
    raw[:, 1:6] = np.frombuffer(b'qrstu', np.uint8) ^ (rng.integers(0, 2, (k, 5)).astype(np.uint8) << 5)
    tails = np.array([list(b'vw'), list(b'Vw'), list(b'vx'), list(b'wv')], dtype=np.uint8)
    which = rng.integers(0, 4, k)
    raw[:, 6:8] = tails[which]
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = IcaseRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, [b'qrstuvw'], texts=False, order=False)
        assert r.last_stats()['hits'] == k > 65536                     # every entry is a candidate
        assert np.array_equal(np.sort(res.ids), np.flatnonzero(which < 2).astype(np.uint64)) and res.ids.size > k // 3
    finally:
        r.close()


@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(140)
    lines = mixed_case_lines(rng, 600, 0, 16)
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = IcaseRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, lines


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """150 patterns of three to seven letters on one chunk expand to 2 048 .. 8 191 spellings and take the 16-lane
    interval search; the switches force the other two."""
    p, ref, lines = shape_index
    search_env(PSS_ICASE_SEED_LETTERS=None, **env)
    rng = np.random.default_rng(141)
    patterns = []
    while len(patterns) < 150:
        ln = lines[int(rng.integers(0, len(lines)))]
        n = int(rng.integers(3, 8))
        if len(ln) >= n:
            at = int(rng.integers(0, len(ln) - n + 1))
            patterns.append(mangle(rng, ln[at:at + n]))
    nvar = sum(len(icase_variants(g)[1]) for g in patterns)
    assert 2048 <= nvar < 8192
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, patterns, interval=R[route])
        assert res.ids.size >= 150 and (res.counts > 0).all()
    finally:
        r.close()


# ---- 9. placement -----------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(142)
    lines = [mangle(rng, b'HEAD%03d ' % i + filler(rng, 6)) if i % 40 == 0 else mangle(rng, filler(rng, int(rng.integers(0, 24))), 0.3)
             for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = IcaseRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'ab', b'BA', b'abc', b'head', b'HEAD0', b'ead12', b'p', b'ponm', b'MISSING', b'd1', b'12', b'0 ']
    patterns += [ch.entry(0).swapcase() for ch in ref.chunks if ch.entry(0)]                    # the entry at offset 0 of every chunk
    patterns += [lines[int(i)][1:8].swapcase() for i in rng.integers(0, len(lines), 30) if len(lines[int(i)]) >= 8]
    # devices=[0, 0]: the merge is part-major inside a pattern, so the stated order is not compared there
    assert H.placement(H.ICASE, p, patterns, search_env, order_multi=False, ref=ref).ids.size > 100


# ---- 10. errors and the conveniences -------------------------------------------------------------------------------------

def test_errors(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        calls = (r.search_icase_batch_packed, r.search_icase_ids_batch, r.count_icase_bytes)
        for call in calls:
            for bad in ([b''], [b'ab', b''], [bytearray()]):
                with pytest.raises(ValueError, match='empty'):
                    call(bad)
            for bad in (b'ab', 'ab', ['ab'], [None]):
                with pytest.raises(TypeError):
                    call(bad)
        # through the C ABI with a reader: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        blob, offs = b'abc', np.array([0, 2, 2, 3], dtype=np.uint64)
        for fn in (_ffi.lib.pss_reader_search_icase_batch, _ffi.lib.pss_reader_search_icase_ids_batch):
            out = ctypes.c_void_p()
            assert fn(h, blob, offs.ctypes.data, 3, ctypes.byref(out)) == _ffi.PSS_EINVAL
            assert not out.value and 'pattern 1 is empty' in _ffi.last_error()
            assert fn(h, blob, offs.ctypes.data, 3, None) == _ffi.PSS_EINVAL
        counts = np.full(4, 7, dtype=np.uint64)
        assert _ffi.lib.pss_reader_count_icase_batch(h, blob, offs.ctypes.data, 3, counts.ctypes.data) == _ffi.PSS_EINVAL
        assert counts.tolist() == [7] * 4 and 'pattern 1 is empty' in _ffi.last_error()
        # ... and a good batch goes through the same call; the reader still answers
        offs = np.array([0, 2, 3], dtype=np.uint64)
        out = ctypes.c_void_p()
        assert _ffi.lib.pss_reader_search_icase_batch(h, blob, offs.ctypes.data, 2, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == ref.search_icase_ids(b'ab').size + ref.search_icase_ids(b'c').size > 0
        _ffi.lib.pss_result_free(out)
        # a pattern with a newline: a count of 0, not an error
        assert r.count_icase_bytes([b'a\nb', b'ab', b'\n']) == [0, ref.search_icase_ids(b'ab').size, 0]
        check(r, ref, [b'AB', b'a\nb', b'c'])
    finally:
        r.close()


def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    w.add_entry('some short string')
    w.add_entry('Another SHORT one')
    w.add_entry('Été short')
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert sorted(r.search('short')) == ['some short string', 'Été short']
        assert sorted(r.search_icase('short')) == sorted(r.search_icase('SHORT')) == sorted(r.search_icase('sHoRt')) == [
            'Another SHORT one', 'some short string', 'Été short']
        assert r.search_icase('SOME SHORT STRING') == ['some short string'] and r.search_icase('shorts') == []
        assert r.count_icase('Short') == 3 and r.count_icase('ANOTHER') == 1 and r.count_icase('short\n') == 0
        # only ASCII letters fold
        assert r.search_icase('ÉTé S') == ['Été short'] and r.search_icase('ÉTÉ') == [] and r.search_icase('été') == [] and r.count_icase('éTé') == 0
        for bad in (b'short', [b'short'], ['short'], None):
            with pytest.raises(TypeError):
                r.search_icase(bad)
            with pytest.raises(TypeError):
                r.count_icase(bad)
        with pytest.raises(ValueError):
            r.search_icase('')
        with pytest.raises(ValueError):
            r.count_icase('')
    finally:
        r.close()
