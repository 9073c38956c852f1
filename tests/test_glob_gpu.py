"""Wildcard search (Reader.search_glob_ids_batch / search_glob_batch_packed / count_glob_bytes and the str conveniences)
against the brute-force reference of tests/glob_ref.py.  Every pattern of every batch goes through one check():
  * per pattern, the sorted ids equal the reference's and no id appears twice; the counts equal the count call's;
  * entry by entry, in order, entries_by_id_packed(ids) is the packed text result (offsets and data), and every entry's
    text is the reference's for its id;
  * the batch took the general pipeline: GENERAL | interval bits (| COUNTS), none of ANCHORED, MID, SMALL_*, RESIDENT,
    SA_ORDER.
The cases: what "in order, without overlap, anchored" means; the LEFTMOST occurrence (two occurrences of a segment inside
one 8-byte word, inside one 64-byte step, in two steps, with the next segment between them -- and the mirror, where only
a found-anywhere check matches); the winning lane's byte offset at every (lane, byte); entry and segment lengths around
the 8- and 64-byte load widths with near misses and exact fits; chunk edges (device hand-over); work that follows the
rarest segment and the tie rule; more candidates than the mid pipeline holds; batch shapes and the three interval routes;
placement (two parts on one device, a shard, a suffix array on the host tier, order='sa', no line table before the id
variant runs); errors and conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, glob_escape, glob_parse
from tests import search_harness as H
from tests.glob_ref import GlobRef
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_pattern

pytestmark = pytest.mark.gpu


def glob(segments, anchors=0):
    """The glob pattern of (segments, anchors)."""
    p = b'*'.join(glob_escape(s) for s in segments)
    p = (b'' if anchors & 1 else b'*') + p + (b'' if anchors & 2 else b'*')
    assert glob_parse(p) == ([bytes(s) for s in segments], anchors)
    return p


def check(r, ref, patterns, **kw):
    """patterns on reader r against ref (the chunks r holds).  Returns the IdResult."""
    return H.check(H.GLOB, r, ref, list(patterns), **kw)


def one_chunk(tmp_path, name, lines):
    data = b'\n'.join(lines) + b'\n'
    assert len(data) < 1_000_000
    p = make_index(tmp_path, name, data)
    ref = GlobRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, data


# ---- 1. meaning ---------------------------------------------------------------------------------------------------

def test_meaning(tmp_path):
    rng = np.random.default_rng(71)
    lines = [b'ERROR TIMEOUT', b'TIMEOUT ERROR', b'ERROR ERROR twice', b'ERROR once', b'A', b'AA', b'ABA', b'ABBA', b'ABXBA', b'XAAY', b'BANANA',
             b'ABABA', b'xABAB', b'GET /x/admin/y 500', b'GET /admin 500 ', b'POST /admin 500', b'500 /admin GET ', b'GET 500 /admin',
             b'T1 T2 T3 T4 T5 T6 T7 T8', b'T1 T2 T3 T4 T5 T6 T7', b'T8 T7 T6 T5 T4 T3 T2 T1', b'T1', b'a*b', b'a\\b', b'axb', b'']
    lines += [filler(rng, int(rng.integers(0, 30))) for _ in range(300)]
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    p, ref, data = one_chunk(tmp_path, 'meaning', lines)
    ts = [b'T%d' % i for i in range(1, 9)]
    patterns = [
        b'*ERROR*TIMEOUT*', b'*TIMEOUT*ERROR*', b'*ERROR*ERROR*', b'*ERROR*',                      # 0 .. 3: order matters; a repeated segment
        b'*A*A*', b'A*A', b'A', b'*A*A*A*', b'AB*BA', b'*AB*BA*', b'*AB*ABA*', b'*A*AB*',            # 4 .. 11: no overlap; a prefix of the next
        b'*A*Y*', b'A*Y*', b'*A*Y', b'X*Y', b'X*A*', b'X*A', b'*X*A',                                # 12 .. 18: the anchors
        b'GET */admin* 500', b'GET */admin*', b'*/admin* 500', b'*GET */admin* 500*',                # 19 .. 22
        b'ABA', b'AB', b'AB*', b'*BA',                                                              # 23 .. 26: one segment
        rb'a\*b', rb'a\\b', b'a*b', rb'*\**',                                                       # 27 .. 30: escapes
        b'*a*b*c*', b'a*', b'*a', b'a*a', b'*ab*ab*', b'*never there*', b'*ERROR*never there*',
    ] + [glob(ts[:k]) for k in range(1, 9)] + [glob(ts[:k], 3) for k in range(1, 9)] + [glob(ts[::-1]), glob(ts[::-1], 3)]
    assert sorted({len(glob_parse(g)[0]) for g in patterns}) == list(range(1, 9))
    r = pysubstringsearch.Reader(p)
    try:
        res = per_pattern(check(r, ref, patterns))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        assert texts(res[0]) == [b'ERROR TIMEOUT'] and texts(res[1]) == [b'TIMEOUT ERROR'] and texts(res[2]) == [b'ERROR ERROR twice']
        assert len(res[3]) == 4
        assert texts(res[4]) == [b'AA', b'ABA', b'ABABA', b'ABBA', b'ABXBA', b'BANANA', b'XAAY', b'xABAB']        # not 'A'
        assert texts(res[5]) == [b'AA', b'ABA', b'ABABA', b'ABBA', b'ABXBA'] and texts(res[6]) == [b'A']
        assert texts(res[7]) == [b'ABABA', b'BANANA']                                                              # needs three
        assert texts(res[8]) == texts(res[9]) == [b'ABABA', b'ABBA', b'ABXBA']                                      # not 'ABA': AB and BA overlap
        assert texts(res[10]) == [b'ABABA'] and texts(res[11]) == [b'ABABA', b'xABAB']
        assert texts(res[12]) == [b'XAAY'] and texts(res[13]) == [] and texts(res[14]) == [b'XAAY'] and texts(res[15]) == [b'XAAY']
        assert texts(res[16]) == [b'XAAY'] and texts(res[17]) == [] and texts(res[18]) == [b'ABXBA']
        assert texts(res[19]) == [b'GET /x/admin/y 500'] and texts(res[20]) == [b'GET /admin 500 ', b'GET /x/admin/y 500', b'GET 500 /admin']
        assert texts(res[21]) == [b'GET /x/admin/y 500', b'POST /admin 500'] and texts(res[22]) == [b'GET /admin 500 ', b'GET /x/admin/y 500']
        assert texts(res[23]) == [b'ABA'] and texts(res[24]) == [] and texts(res[25]) == [b'ABA', b'ABABA', b'ABBA', b'ABXBA']
        assert texts(res[26]) == [b'ABA', b'ABABA', b'ABBA', b'ABXBA']
        assert texts(res[27]) == [b'a*b'] and texts(res[28]) == [b'a\\b'] and {b'a*b', b'a\\b', b'axb'} <= set(texts(res[29])) and texts(res[30]) == [b'a*b']
        at = len(patterns) - 18
        assert texts(res[at + 7]) == [b'T1 T2 T3 T4 T5 T6 T7 T8'] and texts(res[at + 6]) == [b'T1 T2 T3 T4 T5 T6 T7', b'T1 T2 T3 T4 T5 T6 T7 T8']
        assert texts(res[at + 8]) == [b'T1'] and texts(res[at + 8 + 6]) == [b'T1 T2 T3 T4 T5 T6 T7'] and texts(res[at + 8 + 7]) == [b'T1 T2 T3 T4 T5 T6 T7 T8']
        assert texts(res[at + 16]) == texts(res[at + 17]) == [b'T8 T7 T6 T5 T4 T3 T2 T1']
        # *x* is the plain id search, array for array; x with both anchors is the anchored search's 'entry', as a set
        singles = [b'ERROR', b'a', b'ab', b'T1', b'never there', b'ABA', b'p', b'a*b']
        got, plain = check(r, ref, [glob([t]) for t in singles]), r.search_ids_batch(singles)
        assert np.array_equal(got.ids, plain.ids) and np.array_equal(got.counts, plain.counts)
        got, whole = per_pattern(check(r, ref, [glob([t], 3) for t in singles])), r.search_anchored_ids_batch(singles, 'entry')
        assert [sorted(x.tolist()) for x in got] == [sorted(x.tolist()) for x in per_pattern(whole)]
        assert [got[k].size for k in (0, 3, 4, 5, 7)] == [0, 1, 0, 1, 1]
    finally:
        r.close()


PAIRS_AB = ((b'Q', b'R'), (b'SS7', b'TT'), (b'UVWXYZ-UVWXY', b'H' * 9))        # (alphabets of their own, and not the filler's)


# ---- 2. leftmost --------------------------------------------------------------------------------------------------

def test_the_leftmost_occurrence_is_taken(tmp_path):
    """The first segment twice in an entry, the second segment BETWEEN the two and nowhere behind the later one: a walk
    that takes the later occurrence misses.  The two occurrences share an 8-byte word, share a 64-byte step in different
    lanes, or lie in two steps.  The mirror entries hold the second segment only IN FRONT of the first: a check that asks
    "is it anywhere in the entry" matches them wrongly.  Every geometry with one-byte and with longer segments, the entry
    also shifted by 0 .. 3 bytes against the 8-byte grid of the text."""
    rng = np.random.default_rng(72)
    lines, tags = [], []
    geoms = {'word': (0, 3, 6), 'word7': (1, 2, 7), 'step': (3, 21, 40), 'step_adjacent_lanes': (7, 9, 15), 'steps': (3, 70, 140),
             'steps_far': (60, 64, 700)}
    for (A, B) in PAIRS_AB:
        for name, (a1, b, a2) in geoms.items():
            if not (a1 + len(A) <= b and b + len(B) <= a2):
                continue
            for lead in range(4):           # a short entry in front moves the entry's start against the 8-byte grid
                e = bytearray(filler(rng, a2 + len(A) + int(rng.integers(0, 12))))
                e[a1:a1 + len(A)], e[b:b + len(B)], e[a2:a2 + len(A)] = A, B, A
                m = bytearray(filler(rng, len(e)))                      # the mirror: B, then A twice
                m[a1:a1 + len(B)] = B
                m[a2 - len(A):a2], m[a2:a2 + len(A)] = A, A
                lines += [b'z' * lead, bytes(e), bytes(m)]
                tags += [None, (A, B, True), (A, B, False)]
    p, ref, data = one_chunk(tmp_path, 'leftmost', lines)
    r = pysubstringsearch.Reader(p)
    try:
        for (A, B) in PAIRS_AB:
            res = per_pattern(check(r, ref, [glob([A, B]), glob([B, A]), glob([A, B, A]), glob([A, A, B]), glob([B, A, A])]))
            yes = [i for i, t in enumerate(tags) if t == (A, B, True)]
            no = [i for i, t in enumerate(tags) if t == (A, B, False)]
            assert len(yes) == len(no) >= 8
            assert sorted(res[0].tolist()) == yes and sorted(res[2].tolist()) == yes             # A..B..A: *A*B* and *A*B*A*
            assert sorted(res[1].tolist()) == sorted(yes + no) and res[3].size == 0              # B..A both ways round; never A, A, B
            assert sorted(res[4].tolist()) == no
    finally:
        r.close()


def test_the_winning_lanes_byte_offset(tmp_path):
    """The first segment at every (lane, byte) of the first 64-byte step and one position into the second, the second
    segment right behind it -- a position reported too high misses it -- and, in a second entry, a second segment that
    overlaps the first by one byte -- a position reported too low matches it."""
    rng = np.random.default_rng(73)
    lines = []
    for at in range(0, 66):
        e = bytearray(filler(rng, 80))
        e[at:at + 5] = b'QR-RS'               # *QR*-RS* matches (zero gap), *QR*R-* and *QR-*-RS* overlap by one byte
        lines.append(bytes(e))
        e = bytearray(filler(rng, 80))
        e[at:at + 2] = b'QR'                  # and QR without anything behind it
        lines.append(bytes(e))
    p, ref, data = one_chunk(tmp_path, 'offset', lines)
    r = pysubstringsearch.Reader(p)
    try:
        res = per_pattern(check(r, ref, [b'*QR*-RS*', b'*QR*R-*', b'*QR-*-RS*', b'*Q*R*-*R*S*', b'*QR*QR*', b'*QR-RS*', b'*QR*']))
        even = list(range(0, 132, 2))
        assert sorted(res[0].tolist()) == sorted(res[3].tolist()) == sorted(res[5].tolist()) == even
        assert res[1].size == res[2].size == res[4].size == 0 and res[6].size == 132
    finally:
        r.close()


# ---- 3. entry and segment lengths around the load widths ----------------------------------------------------------------

ENTRY_LENS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 300, 5000)
SEG_LENS = (1, 7, 8, 9, 64, 300)
PAIRS = sorted({(a, b) for a in SEG_LENS for b in (1, 9)} | {(a, b) for a in (1, 9) for b in SEG_LENS})


def test_entry_and_segment_lengths_around_the_load_widths(tmp_path):
    """T_m and U_m are prefixes of two 300-byte strings over alphabets the filler lacks.  For every pair of lengths in
    PAIRS and every entry length that holds both, T sits at the start (or 3 bytes in) and U begins right behind T (the
    walk's `from` is unaligned, the gap zero), across an 8-byte and across a 64-byte position counted from there, or at
    the very end of the entry -- and beside every such entry stands its near miss, U with the last byte changed.  Exact
    fits: the entry T + U (the lengths sum to the entry's), and T + U[:-1], which starts with T and ends with
    Y = T[-1] + U[:-1], one byte more than the entry has: T*Y overlaps by one byte under every anchor combination."""
    rng = np.random.default_rng(74)
    base_t = bytes(np.frombuffer(b'QRSTUVWXY', np.uint8)[rng.integers(0, 9, 300)])
    base_u = bytes(np.frombuffer(b'HIJKLMNOZ', np.uint8)[rng.integers(0, 9, 300)])
    T = {m: base_t[:m] for m in SEG_LENS}
    U = {m: base_u[:m] for m in SEG_LENS}
    Y = {(a, b): T[a][-1:] + U[b][:-1] for a, b in PAIRS}
    lines = [filler(rng, n) for n in ENTRY_LENS for _ in range(2)]
    lines += [T[m] for m in SEG_LENS] + [T[m] + b'x' for m in SEG_LENS] + [b'x' + T[m] for m in SEG_LENS]       # one segment, both anchors
    planted = 0
    for (a, b) in PAIRS:
        lines += [T[a] + U[b], T[a] + U[b][:-1], T[a] + b'x' + U[b], U[b] + T[a]]
        for n in ENTRY_LENS:
            for at1 in (0, 3):
                frm = at1 + a
                places = {'behind': frm, 'end': n - b}
                if at1 == 0:
                    places.update(x8=frm + max(1, 8 - (b + 1) // 2), x64=frm + max(1, 64 - (b + 1) // 2))
                if n == 5000:
                    places = {'end': n - b} if at1 == 0 else {}
                for u_at in sorted(set(places.values())):
                    if u_at < frm or u_at + b > n:
                        continue
                    for u in (U[b], U[b][:-1] + b'!'):
                        e = bytearray(filler(rng, n))
                        e[at1:at1 + a] = T[a]
                        e[u_at:u_at + b] = u
                        lines.append(bytes(e))
                        planted += 1
    p, ref, data = one_chunk(tmp_path, 'widths', lines)
    assert planted > 600
    patterns = [glob([T[m]], 3) for m in SEG_LENS] + [glob([T[m]], 1) for m in SEG_LENS] + [glob([T[m]], 2) for m in SEG_LENS]
    for (a, b) in PAIRS:
        patterns += [glob([T[a], U[b]], k) for k in range(4)] + [glob([T[a], Y[a, b]], k) for k in range(4)] + [glob([U[b], T[a]], 0)]
    r = pysubstringsearch.Reader(p)
    try:
        res = per_pattern(check(r, ref, patterns))
        texts = lambda ids: sorted(r.entries_by_id(ids))
        for k, m in enumerate(SEG_LENS):
            assert set(texts(res[k])) == {T[m]} and T[m] + b'x' in texts(res[6 + k]) and b'x' + T[m] in texts(res[12 + k])
        for k, (a, b) in enumerate(PAIRS):
            any_, start, end, both, y_any, y_start, y_end, y_both, rev = res[18 + 9 * k:18 + 9 * k + 9]
            fit = T[a] + U[b]
            assert fit in texts(both) and T[a] + b'x' + U[b] in texts(both) and both.size >= 3, (a, b)
            assert set(both.tolist()) <= set(start.tolist()) <= set(any_.tolist()) and set(both.tolist()) <= set(end.tolist()) <= set(any_.tolist())
            if a + b <= 128:                 # (a 300-byte segment fits the 5000-byte entries alone)
                assert any_.size > start.size > both.size and any_.size > end.size > both.size, (a, b)
            # T + U[:-1] starts with T and ends with Y, one byte short of holding both
            assert all(T[a] + U[b][:-1] not in texts(y) for y in (y_any, y_start, y_end, y_both)), (a, b)
            assert U[b] + T[a] in texts(rev) and fit not in texts(rev), (a, b)
    finally:
        r.close()


# ---- 4. chunk edges ---------------------------------------------------------------------------------------------------

def test_chunk_edges_handed_over_on_the_device():
    texts = [b'ONLYONE x\n',                         # 0: a one-entry chunk
             b'first x\n\n\nab\nmid x\nx NOEND',      # 1: the entry at offset 0, empty entries, a short entry, no closing newline
             b'NOEND',                               # 2: the whole chunk is one unterminated entry
             b'\n', b'x',                            # 3, 4
             b'xb\x00y\nab',                         # 5: a real 0x00, and 'b' as the very last byte before the padding
             b'b',                                   # 6
             b'ONLYA here\nx\n', b'ONLYB here\nx\n',  # 7, 8: two segments that never share a chunk
             b'HEL\nLO x\nHELLO']                    # 9
    ref = GlobRef(texts)
    r = device_reader(texts)
    try:
        patterns = [
            # the entry at offset 0 with START
            b'first*', b'first*x', b'f*t*x', b'*first*x*', b'irst*', b'ONLYONE*x', b'ONLYONE x', b'O*E*x', b'*x*ONLYONE*', b'mid*x', b'a*b', b'ab', b'a*',
            # the unterminated last entry: END, and the last byte takes part
            b'*NOEND', b'x*NOEND', b'*NOEN', b'x*D', b'*x*N*D', b'*N*D*', b'NOEND', b'N*D', b'NOEN', b'NOEN*', b'*NO*END', b'*NOE*END', b'*NOEND*D*',
            b'*D', b'*x*NOENDx*', b'x', b'*x', b'x*',
            # 0x00: in the text it matches, against the zero padding behind the chunk it does not
            b'*b*\x00*', b'*b\x00*', b'*b*\x00', b'*x*\x00*y', b'x*\x00*', b'*a*b*\x00*', b'b*\x00', b'*b\x00\x00*', b'*\x00*', b'b', b'*b',
            b'*x*\x00*', b'*D*\x00\x00\x00\x00\x00\x00\x00\x00\x00*', b'*N*D\x00*',
            # 0x0A: a segment with one voids its pattern
            b'*x*\n*', b'*\n*x*', b'*\n*', b'*HEL*\nLO*', b'*HEL\nLO*', b'HEL\n*', b'*HEL*LO*', b'HEL*LO', b'*LO*HEL*', b'*x\n', b'first x\n*',
            b'*ONLYA*here*', b'*ONLYB*here', b'*here*x*', b'*here',
        ]
        res = per_pattern(check(r, ref, patterns))
        at = {g: i for i, g in enumerate(patterns)}
        noend = [(1 << 32) | 5, 2 << 32]
        assert res[at[b'first*']].tolist() == res[at[b'first*x']].tolist() == res[at[b'f*t*x']].tolist() == [1 << 32] and res[at[b'irst*']].size == 0
        assert res[at[b'ONLYONE*x']].tolist() == res[at[b'ONLYONE x']].tolist() == res[at[b'O*E*x']].tolist() == [0] and res[at[b'*x*ONLYONE*']].size == 0
        assert sorted(res[at[b'*NOEND']].tolist()) == sorted(res[at[b'*N*D*']].tolist()) == sorted(res[at[b'*NO*END']].tolist()) == noend
        assert res[at[b'x*NOEND']].tolist() == res[at[b'x*D']].tolist() == res[at[b'*x*N*D']].tolist() == [noend[0]]
        assert res[at[b'NOEND']].tolist() == res[at[b'N*D']].tolist() == [noend[1]]
        assert res[at[b'*NOEN']].size == res[at[b'NOEN']].size == res[at[b'*NOE*END']].size == res[at[b'*NOEND*D*']].size == 0
        assert res[at[b'NOEN*']].tolist() == [noend[1]] and sorted(res[at[b'*D']].tolist()) == noend
        assert r.entries_by_id(noend) == [b'x NOEN', b'NOEN']          # handed out without the last byte, matched with it
        assert sorted(res[at[b'x']].tolist()) == [4 << 32, (7 << 32) | 1, (8 << 32) | 1]             # the one-byte chunk 'x' too
        assert res[at[b'*b*\x00*']].tolist() == res[at[b'*b\x00*']].tolist() == res[at[b'*x*\x00*y']].tolist() == res[at[b'x*\x00*']].tolist() == [5 << 32]
        assert res[at[b'*b*\x00']].size == res[at[b'*a*b*\x00*']].size == res[at[b'b*\x00']].size == res[at[b'*b\x00\x00*']].size == 0
        assert res[at[b'*\x00*']].tolist() == [5 << 32] and res[at[b'*N*D\x00*']].size == 0
        assert sorted(res[at[b'b']].tolist()) == [6 << 32] and sorted(res[at[b'*b']].tolist()) == [(1 << 32) | 3, (5 << 32) | 1, 6 << 32]
        for g in (b'*x*\n*', b'*\n*x*', b'*\n*', b'*HEL*\nLO*', b'*HEL\nLO*', b'HEL\n*', b'*x\n', b'first x\n*'):
            assert res[at[g]].size == 0, g
        assert res[at[b'*HEL*LO*']].tolist() == res[at[b'HEL*LO']].tolist() == [(9 << 32) | 2] and res[at[b'*LO*HEL*']].size == 0
        # segments that occur only in different chunks: no hit is looked at
        got = check(r, ref, [b'*ONLYA*ONLYB*', b'ONLYB here*ONLYA', b'*ONLYB*ONLYA*x*'])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
        assert r.count_glob_bytes([b'*ONLYA*ONLYB*']) == [0] and r.last_stats()['hits'] == 0
        # ... nor for a pattern that a newline voids, however often its other segments occur
        got = check(r, ref, [b'*x*\n*', b'x*x\nx'])
        assert got.ids.size == 0 and r.last_stats()['hits'] == 0
    finally:
        r.close()


# ---- 5. the work follows the rarest segment -----------------------------------------------------------------------------

def test_hits_follow_the_rarest_segment(tmp_path):
    """'a' occurs about 50 times in each of 300 entries, 'RARE' once in 12 of them: wherever it stands in the pattern,
    the batch looks at the hits of RARE alone.  Both figures come from the text."""
    rng = np.random.default_rng(75)
    lines = []
    for i in range(300):
        body = np.frombuffer(b'ab', np.uint8)[rng.integers(0, 2, 100)].tobytes()
        lines.append(body[:40] + b'RARE' + body[40:] if i % 25 == 0 else body)
    # a tie: TIEX and TIEY occur four times each, in the same four entries, in different suffix orders
    lines += [b'TIEX1 TIEY2', b'TIEX2 TIEY1', b'TIEY3 TIEX4', b'TIEY4 TIEX3']
    p, ref, data = one_chunk(tmp_path, 'work', lines)
    rare = data.count(b'RARE')
    assert rare == 12 and data.count(b'TIEX') == data.count(b'TIEY') == 4
    r = pysubstringsearch.Reader(p)
    try:
        for pat in (b'*a*RARE*', b'*RARE*a*', b'*a*b*RARE*ab*', b'*a*RARE*a*'):
            got = check(r, ref, [pat])
            assert got.ids.size == rare and r.last_stats()['hits'] == rare
            assert r.count_glob_bytes([pat]) == [rare] and r.last_stats()['hits'] == rare
            assert len(r.search_glob_batch_packed([pat]).counts) == 1 and r.last_stats()['hits'] == rare
        assert r.count_multiple_bytes([b'a']) == [300]
        assert r.last_stats()['hits'] == data.count(b'a') >= 20 * rare
        # equal counts: the segment with the lowest index drives, and its plain order is the pattern's
        x, y = r.search_ids_batch([b'TIEX']).ids.tolist(), r.search_ids_batch([b'TIEY']).ids.tolist()
        n0 = 300
        assert sorted(x) == sorted(y) == [n0, n0 + 1, n0 + 2, n0 + 3]
        xy, yx = [n0, n0 + 1], [n0 + 2, n0 + 3]                             # the entries with X before Y, and with Y before X
        in_order = lambda order, keep: [i for i in order if i in keep]
        assert in_order(x, xy) != in_order(y, xy) and in_order(x, yx) != in_order(y, yx)          # (so the driver shows)
        assert check(r, ref, [b'*TIEX*TIEY*']).ids.tolist() == in_order(x, xy)
        assert check(r, ref, [b'*TIEY*TIEX*']).ids.tolist() == in_order(y, yx)
        assert check(r, ref, [b'TIEY*TIEX*']).ids.tolist() == in_order(y, yx) and r.last_stats()['hits'] == 4
    finally:
        r.close()


# ---- 6. more candidates than the mid pipeline's 65 536 and than one scan workgroup -----------------------------------

def test_more_candidates_than_the_mid_pipeline_holds(tmp_path):
    rng = np.random.default_rng(76)
    k = 70000
    raw = np.full((k, 3), 0x0A, dtype=np.uint8)
    xa = rng.integers(0, 2, k).astype(bool)
    raw[:, 0] = np.where(xa, ord('x'), ord('a'))
    raw[:, 1] = np.where(xa, ord('a'), ord('x'))
    data = raw.tobytes()
    p = make_index(tmp_path, 'many', data)
    ref = GlobRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    r = pysubstringsearch.Reader(p)
    try:
        res = per_pattern(check(r, ref, [b'*x*a*', b'a*x', b'*x*'], texts=False))
        assert r.last_stats()['hits'] == 3 * k                       # every entry is a candidate of every pattern
        assert np.array_equal(np.sort(res[0]), np.flatnonzero(xa).astype(np.uint64)) and res[0].size > k // 3
        assert np.array_equal(np.sort(res[1]), np.flatnonzero(~xa).astype(np.uint64)) and res[2].size == k > 65536
    finally:
        r.close()


# ---- 7. batch shapes and interval routes ------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shape_index(tmp_path_factory):
    rng = np.random.default_rng(77)
    lines = [filler(rng, int(rng.integers(0, 10))) for _ in range(600)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path_factory.mktemp('shape'), 'shape', data)
    ref = GlobRef.from_index(p)
    assert [ch.text for ch in ref.chunks] == [data]
    return p, ref, lines


def test_batch_shapes(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, [])
        assert res.ids.size == 0 and res.counts.size == 0
        assert r.search_glob_batch_packed([]).offsets.tolist() == [0] and r.count_glob_bytes([]) == []
        res = check(r, ref, [b'*MISS*', b'*a*MISS*', b'*MISS*a*', b'MISS', b'*\x01*a', b'*' + b'Z' * 40 + b'*zz*'])
        assert res.ids.size == 0 and res.counts.tolist() == [0] * 6 and r.last_stats()['hits'] == 0
        res = check(r, ref, [b'*a*', b'*MISS*', b'*a*b*', b'*b*a*', b'a*', b'*a'], interval=R['INTERVAL_WAVE'])
        assert res.counts[0] > res.counts[2] > 0 and res.counts[3] > 0 and res.counts[1] == 0 and res.counts[4] > 0 and res.counts[5] > 0
    finally:
        r.close()


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(shape_index, search_env, route, env):
    """3 000 patterns of one to three segments on one chunk (about 6 000 segment pairs) take the 16-lane interval search;
    the switches force the other two."""
    p, ref, lines = shape_index
    search_env(**env)
    rng = np.random.default_rng(78)

    def pieces(k):
        ln = lines[int(rng.integers(0, len(lines)))]
        if len(ln) < 2 * k or rng.integers(0, 8) == 0:
            return [filler(rng, 1) for _ in range(k)]
        cuts = np.sort(rng.choice(len(ln) + 1, 2 * k, replace=False)).tolist()       # k pieces of one entry, in order
        return [ln[cuts[2 * i]:cuts[2 * i + 1]] for i in range(k)]

    patterns = [glob(pieces(1 + i % 3), int(rng.choice(4, p=[0.55, 0.15, 0.15, 0.15]))) for i in range(3000)]
    nseg = sum(len(glob_parse(g)[0]) for g in patterns)
    assert 2048 <= nseg < 8192
    r = pysubstringsearch.Reader(p)
    try:
        res = check(r, ref, patterns, interval=R[route])
        assert res.ids.size > 1000 and (res.counts == 0).sum() > 100
    finally:
        r.close()


# ---- 8. placement -----------------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(79)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = GlobRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'*a*b*', b'*b*a*', b'a*b', b'HEAD*0*', b'*HEAD*a*b*', b'*p*', b'*ab*cd*', b'*a*b*c*d*', b'*MISS*a*', b'e*', b'*e', b'HEAD*']
    patterns += [glob([ch.entry(0)], 3) for ch in ref.chunks if ch.entry(0)]                    # the entry at offset 0 of every chunk
    patterns += [glob([lines[int(i)][:2], lines[int(i)][-2:]], int(rng.integers(0, 4))) for i in rng.integers(0, len(lines), 30)
                 if len(lines[int(i)]) >= 4]
    assert H.placement(H.GLOB, p, patterns, search_env, ref=ref).ids.size > 100


# ---- 9. errors and the conveniences -------------------------------------------------------------------------------------

def c_batch(segs, goff, anch):
    blob = b''.join(segs)
    offs = np.cumsum([0] + [len(t) for t in segs]).astype(np.uint64)
    return blob, offs, np.array(goff, dtype=np.uint64), np.array(anch if anch else [0], dtype=np.uint8)


BAD_C_BATCHES = [
    ('no segment', [b'a', b'b'], [0, 0, 2], [0, 0]),
    ('no segment', [b'a'], [0, 1, 1], [3, 3]),
    ('is empty', [b'a', b''], [0, 2], [0]),
    ('anchors[0] = 4', [b'a', b'b'], [0, 2], [4]),
    ('anchors[1] = 255', [b'a', b'b'], [0, 1, 2], [3, 255]),
    ('group offsets', [b'a', b'b'], [1, 2], [0]),
    ('group offsets', [b'a', b'b'], [0, 1], [0]),
    ('group offsets', [b'a', b'b', b'c'], [0, 2, 1, 3], [0, 0, 0]),
    ('group offsets', [b'a', b'b'], [0, 3, 2], [0, 0]),
]


def test_errors(shape_index):
    p, ref, lines = shape_index
    r = pysubstringsearch.Reader(p)
    try:
        calls = (r.search_glob_batch_packed, r.search_glob_ids_batch, r.count_glob_bytes)
        for call in calls:
            for bad, what in (([b'*'], 'no literal byte'), ([b'a*b', b''], 'no literal byte'), ([b'a\\'], 'lone backslash')):
                with pytest.raises(ValueError, match=what):
                    call(bad)
            for bad in (b'a*b', 'a*b', ['a*b']):
                with pytest.raises(TypeError):
                    call(bad)
        # through the C ABI: PSS_EINVAL with a message, *out and counts untouched
        h = r._handle()
        for what, segs, goff, anch in BAD_C_BATCHES:
            blob, offs, g, a = c_batch(segs, goff, anch)
            ng = len(goff) - 1
            for fn in (_ffi.lib.pss_reader_search_seq_batch, _ffi.lib.pss_reader_search_seq_ids_batch):
                out = ctypes.c_void_p()
                assert fn(h, blob, offs.ctypes.data, len(segs), g.ctypes.data, ng, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value and what in _ffi.last_error(), (what, _ffi.last_error())
            counts = np.full(4, 7, dtype=np.uint64)
            assert _ffi.lib.pss_reader_count_seq_batch(h, blob, offs.ctypes.data, len(segs), g.ctypes.data, ng, a.ctypes.data,
                                                       counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
        # a null out, null offsets, null anchors
        blob, offs, g, a = c_batch([b'a', b'b'], [0, 2], [0])
        args = (h, blob, offs.ctypes.data, 2, g.ctypes.data, 1, a.ctypes.data)
        assert _ffi.lib.pss_reader_search_seq_batch(*args, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_seq_ids_batch(*args, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_count_seq_batch(*args, None) == _ffi.PSS_EINVAL
        out = ctypes.c_void_p()
        assert _ffi.lib.pss_reader_search_seq_batch(h, blob, offs.ctypes.data, 2, None, 1, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_seq_batch(h, blob, offs.ctypes.data, 2, g.ctypes.data, 1, None, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_search_seq_batch(h, blob, None, 2, g.ctypes.data, 1, a.ctypes.data, ctypes.byref(out)) == _ffi.PSS_EINVAL
        assert not out.value
        # ... and the good batch goes through the same call; the reader still answers
        assert _ffi.lib.pss_reader_search_seq_batch(*args, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == ref.search_seq_ids([b'a', b'b'], 0).size > 0
        _ffi.lib.pss_result_free(out)
        check(r, ref, [b'*a*b*', b'a*b'])
        # an all-terms batch still wants its exclude flags
        assert _ffi.lib.pss_reader_search_terms_batch(h, blob, offs.ctypes.data, 2, g.ctypes.data, 1, None, ctypes.byref(out)) == _ffi.PSS_EINVAL
    finally:
        r.close()


def test_conveniences_on_the_readme_example(tmp_path):
    p = str(tmp_path / 'out.idx')
    w = pysubstringsearch.Writer(p)
    w.add_entry('some short string')
    w.finalize()
    w.close()
    r = pysubstringsearch.Reader(p)
    try:
        assert r.search('short') == ['some short string']
        assert r.search_glob('some*string') == r.search_glob('*short*') == r.search_glob('s*s*s*g') == ['some short string']
        assert r.search_glob('*some*short*string*') == r.search_glob('some short string') == r.search_glob('*o*o*') == ['some short string']
        assert r.search_glob('*string*short*') == [] and r.search_glob('short*') == [] and r.search_glob('*short') == []
        assert r.search_glob('some*some*') == [] and r.search_glob('*string*g') == [] and r.search_glob('some short string*g') == []
        assert r.search_glob('some\\*string') == [] and r.search_glob('some short strin') == []
        assert r.count_glob('some*') == 1 and r.count_glob('*string') == 1 and r.count_glob('*s*s*s*s*') == 0 and r.count_glob('*s*s*s*') == 1
        for bad in (b'some*', [b'some*'], ['some*'], None):
            with pytest.raises(TypeError):
                r.search_glob(bad)
            with pytest.raises(TypeError):
                r.count_glob(bad)
        for bad in ('', '*', '**', 'some\\'):
            with pytest.raises(ValueError):
                r.search_glob(bad)
            with pytest.raises(ValueError):
                r.count_glob(bad)
    finally:
        r.close()


def test_rows_and_segment_bytes_around_a_multiple_of_64():
    """63, 64 and 65 patterns whose segment bytes add up to 31, 32 and 33 modulo 64, on one chunk and on three (search_harness.layout_edges)."""
    H.layout_edges(H.GLOB, H.edge_globs, min_ids=63)
