"""Wildcard search with byte classes (Reader.search_glob_ids_batch / search_glob_batch_packed / count_glob_bytes and the
str conveniences under classes=True) against the brute-force reference of tests/glob_class_ref.py.  Every batch goes
through the check() of tests/search_harness.py with a Kind of this suite's own, exact and under icase=True: ids, counts,
packed text, routes and `hits` are all held to the reference.
The cases: what `?`, a set and a negated set mean; where the core sits inside its segment and how far the class positions
around it may reach (from, lim, the entry's two ends); the retry when an occurrence of the core fails a class position
(overlapping occurrences, one word, one step, two steps, a mirror); segments without a core; entry and segment lengths
around the 8- and 64-byte load widths; chunk edges (device hand-over); fold; work that follows the rarest core and the tie
rule; the order; more candidates than the mid pipeline holds; placement; the three interval routes; errors and
conveniences."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi, glob_cores, glob_escape
from tests import search_harness as H
from tests.glob_class_ref import GlobClassRef, occurrences
from tests.glob_ref import GlobRef
from tests.search_harness import R, device_reader, filler, make_index, per_row as per_pattern
from tests.test_glob_class_host import BAD_C_BATCHES, c_args

pytestmark = pytest.mark.gpu


def _kind(fold):
    return H.Kind('glob_class_icase' if fold else 'glob_class', GlobClassRef,
                  ids=lambda r, b: r.search_glob_ids_batch(b, classes=True, icase=fold),
                  packed=lambda r, b: r.search_glob_batch_packed(b, classes=True, icase=fold),
                  counts=lambda r, b: r.count_glob_bytes(b, classes=True, icase=fold),
                  rows=H._listed, want=lambda ref, p: ref.search_glob_ids(p, fold),
                  want_hits=lambda ref, b: ref.hits(b, fold))


CLASS, CLASS_ICASE = _kind(False), _kind(True)


def check(r, ref, patterns, **kw):
    """patterns on reader r against ref, exact and under fold.  Returns the exact IdResult."""
    res = H.check(CLASS, r, ref, list(patterns), **kw)
    H.check(CLASS_ICASE, r, ref, list(patterns), **kw)
    return res


def one_chunk(lines, closed=True):
    return H.one_chunk(GlobClassRef, lines, closed)


def texts_of(r, ids):
    return sorted(r.entries_by_id(ids))


def cls(rng, n):
    """n class positions that accept every byte of the filler alphabet (a .. p): `?`, a range, a negated set."""
    return b''.join((b'?', b'[a-p]', b'[!Q\\]]', b'[\\a-\\p]')[int(i)] for i in rng.integers(0, 4, n))


# ---- 1. meaning ---------------------------------------------------------------------------------------------------

def test_meaning():
    rng = np.random.default_rng(181)
    lines = [b'ac', b'abc', b'abbc', b'Z', b'Y', b'ab', b'a', b'a?[b]', b'a?c', b'user=1234 x', b'user=12a4 x', b'user=123 x', b'id=abcd-ef9',
             b'id=abc-def', b'GET /api/v2 503', b'GET /api/v2 505', b'GET /api/v12 500', b'GET /api/v1 500', b'x^y', b'x!y', b'x-y', b'x]y', b'xay',
             b'k\xc1z', b'k\xe1z', b'']
    lines += [filler(rng, int(rng.integers(0, 30))) for _ in range(200)]
    r, ref, data = one_chunk(lines)
    patterns = [b'a?c', b'a*?', b'*a*?', b'Z?Y', b'Z[!x]Y', b'*Z[!x]Y*',                                   # 0 .. 5
                b'*user=[0-9][0-9][0-9][0-9] *', b'*id=????-??*', b'GET /api/v? 50[0-4]',                  # 6 .. 8
                b'x[\\^!]y', b'x[!^!]y', b'x[]-]y', b'x[a-a]y', b'x[!a-z]y', b'k[\xc0-\xc2]z', b'*[!a-p]*c*',   # 9 .. 15
                b'a\\?\\[b\\]', b'a?[b]*', b'?b?', b'a?', b'?a*']
    try:
        res = per_pattern(check(r, ref, patterns))
        t = lambda i: texts_of(r, res[i])
        assert t(0) == [b'a?c', b'abc']                                        # `?` is exactly one byte: neither ac nor abbc
        assert b'a' not in t(1) and b'ab' in t(1) and b'ac' in t(1)            # a*? needs a byte behind the a
        assert t(3) == [] and t(4) == [] and t(5) == []                        # the entries Z and Y: nothing reaches over the newline
        assert t(6) == [b'user=1234 x'] and t(7) == [b'id=abcd-ef9'] and t(8) == [b'GET /api/v1 500', b'GET /api/v2 503']
        assert t(9) == [b'x!y', b'x^y'] and t(10) == [b'x-y', b'x]y', b'xay'] and t(11) == [b'x-y', b'x]y'] and t(12) == [b'xay']
        assert t(13) == [b'x!y', b'x-y', b'x]y', b'x^y'] and t(14) == [b'k\xc1z']
        assert t(16) == [b'a?[b]'] and b'a?[b]' not in t(17) and b'abbc' in t(17) and {b'ab', b'ac'} <= set(t(19)) and b'a' not in t(19)
        # patterns without specials: the identical id arrays with and without the keyword
        plain = [b'*a*b*', b'a*c', b'*user=*x', b'GET*500', b'*never there*', b'ab', b'*p*p*']
        for fold in (False, True):
            a = r.search_glob_ids_batch(plain, classes=True, icase=fold)
            b = r.search_glob_ids_batch(plain, icase=fold)
            assert np.array_equal(a.ids, b.ids) and np.array_equal(a.counts, b.counts) and a.ids.size > 5
        # ... and without the keyword `?`, `[` and `]` are bytes
        got = per_pattern(r.search_glob_ids_batch([b'a?[b]', b'*?[*', b'a?c']))
        assert [texts_of(r, g) for g in got] == [[b'a?[b]'], [b'a?[b]'], [b'a?c']]
        assert r.search_glob('a?c') == ['a?c'] and sorted(r.search_glob('a?c', classes=True)) == ['a?c', 'abc']
    finally:
        r.close()


# ---- 2. where the core sits ----------------------------------------------------------------------------------------

CORE_OFFSETS = (0, 1, 7, 8, 9, 63, 64, 65)


def test_the_cores_offset_and_the_reach_of_the_class_positions():
    """A segment of k class positions, the core QRS and t more class positions, under every anchor combination and between
    two other segments: the entries hold k - 1, k and k + 1 bytes in front of the core and t - 1, t and t + 1 behind it, so
    the class positions reach exactly to `from` / `lim` / the entry's ends, or one byte past them -- into the piece before,
    the piece behind, the previous entry or the closing newline."""
    rng = np.random.default_rng(182)
    lines, patterns = [], []
    for k in CORE_OFFSETS:
        for t in (0, 1, 9):
            seg = cls(rng, k) + b'QRS' + cls(rng, t)
            assert glob_cores(seg) == [(k, b'QRS')]
            patterns += [b'*' + seg + b'*', seg + b'*', b'*' + seg, seg, b'AB*' + seg + b'*YZ', b'AB' + seg + b'YZ*', b'*Y*' + seg]
            for pre in (k - 1, k, k + 1):
                for post in (t - 1, t, t + 1):
                    if pre < 0 or post < 0:
                        continue
                    body = filler(rng, pre) + b'QRS' + filler(rng, post)
                    lines += [body, b'AB' + body + b'YZ', b'Y' + body]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, patterns)
        assert (res.counts > 0).all() and res.counts.sum() < len(lines) * len(patterns) // 8
    finally:
        r.close()


# ---- 3. the retry --------------------------------------------------------------------------------------------------

def test_the_next_occurrence_of_the_core_is_tried():
    """The core twice or more in an entry, the first occurrence failing a class position: the two share an 8-byte word,
    share a 64-byte step in different lanes, or lie in two steps; overlapping occurrences; and mirrors that hold the core
    and, elsewhere, a byte of the set -- what a "both are somewhere" check would accept."""
    rng = np.random.default_rng(183)
    lines = [b'ZZZZ', b'ZZZY', b'ZZY', b'ZZ', b'YZZZ', b'ZZZZY ZZZZ', b'QR5', b'QRx', b'QRQR5', b'QRQRQRx', b'5QR', b'QRx5', b'QR x 5 QR']
    geoms = {'word': (0, 3), 'word7': (1, 5), 'step': (3, 40), 'adjacent_lanes': (6, 9), 'steps': (3, 70), 'steps_far': (60, 700)}
    for name, (a1, a2) in geoms.items():
        for lead in range(4):               # a short entry in front moves the entry's start against the 8-byte grid
            e = bytearray(filler(rng, a2 + 3 + int(rng.integers(0, 12))))
            e[a1:a1 + 3], e[a2:a2 + 3] = b'QRx', b'QR5'
            m = bytearray(e)                # the mirror: the digit behind neither occurrence
            m[a2:a2 + 3] = b'QRy'
            m[a1 + 3:a1 + 4] = b'x'
            m2 = bytes(m) + b'5'
            w = bytearray(e)                # the other way round: the first occurrence fits
            w[a1:a1 + 3], w[a2:a2 + 3] = b'QR5', b'QRx'
            lines += [b'z' * lead, bytes(e), bytes(m), m2, bytes(w)]
    r, ref, data = one_chunk(lines)
    patterns = [b'*ZZ[!Z]*', b'ZZ[!Z]', b'*ZZ[!Z]', b'*[!Z]ZZ*', b'*ZZ[Y]*', b'*Z[Z]Z?*', b'*QR[0-9]*', b'*QR[0-9]', b'QR[0-9]*', b'*[0-9]QR*',
                b'*QR[!a-z]*', b'*Q?[0-9]*', b'*QR[0-9]*QR[a-z]*', b'*QR[a-z]*QR[0-9]*', b'*QR?*5*']
    try:
        res = per_pattern(check(r, ref, patterns))
        assert texts_of(r, res[0]) == [b'ZZY', b'ZZZY', b'ZZZZY ZZZZ'] and texts_of(r, res[1]) == [b'ZZY'] and texts_of(r, res[2]) == [b'ZZY', b'ZZZY']
        assert res[6].size >= 2 + 2 * 4 * len(geoms) and res[6].size < res[14].size
    finally:
        r.close()


# ---- 4. segments without a core ------------------------------------------------------------------------------------

def test_segments_without_a_core():
    rng = np.random.default_rng(184)
    lines = [b'ab', b'axb', b'axyb', b'axyzb', b'axyzwb', b'a', b'b', b'ax', b'axy', b'xa', b'xya', b'xyaz', b'a12b', b'a1b2', b'a1x2b', b'12ab', b'ab12']
    for i in range(0, 67):                  # the two digits at every (lane, byte) of a step, and one step further
        lines += [b'a' + filler(rng, i) + b'42' + filler(rng, int(rng.integers(0, 5))) + b'b',
                  b'a' + filler(rng, i) + b'4x2' + filler(rng, 3) + b'b', b'a' + filler(rng, i) + b'b42']
    r, ref, data = one_chunk(lines)
    patterns = [b'a*???*b', b'*a*???*b*', b'a*[0-9][0-9]*b', b'*a*[0-9][0-9]*b*', b'a*??', b'??*a', b'*??*a*', b'a*??*b', b'a*?*b', b'a*[!x]?*b',
                b'??*a*??', b'[0-9]?*a*', b'*a*[0-9]', b'a*[a-p][0-9]*b', b'a*?[0-9][0-9]?*b', b'?*a']
    try:
        res = per_pattern(check(r, ref, patterns))
        assert b'axyb' not in texts_of(r, res[0]) and b'axyzb' in texts_of(r, res[0])           # gaps of 2, 3 and 4 bytes
        assert b'axyb' in texts_of(r, res[7]) and b'axb' not in texts_of(r, res[7])             # an exact fit, and one byte short
        assert res[2].size >= 67 + 1
    finally:
        r.close()


# ---- 5. lengths ------------------------------------------------------------------------------------------------------

ENTRY_LENS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 300)
SEGMENT_LENS = (1, 7, 8, 9, 64, 300)


def test_entry_and_segment_lengths_around_the_load_widths():
    rng = np.random.default_rng(185)
    lines = [filler(rng, n) for n in ENTRY_LENS for _ in range(3)]
    patterns = []
    for L in SEGMENT_LENS:
        W = b'R' + filler(rng, L - 1)
        for i in sorted({0, L - 1, 7, 8} & set(range(L))):
            if L == 1:
                continue
            for c in (b'?', b'[' + glob_escape(W[i:i + 1], classes=True) + b'Z]', b'[!Z]'):
                seg = glob_escape(W[:i], classes=True) + c + glob_escape(W[i + 1:], classes=True)
                patterns += [seg, b'*' + seg, seg + b'*', b'*' + seg + b'*']
            miss = W[:i] + b'Z' + W[i + 1:]                                    # differs in the class position only
            keep = W[:i] + b'q' + W[i + 1:]
            for n in ENTRY_LENS:
                for body in (W, miss, keep):
                    lines += [body, filler(rng, n) + body, body + filler(rng, n), filler(rng, n)[:n // 2] + body + filler(rng, n)[n // 2:]]
        patterns += [b'*' + glob_escape(W, classes=True) + b'*?', b'?*' + glob_escape(W, classes=True), b'*?' + glob_escape(W, classes=True) + b'?*']
        lines += [W, b'x' + W, W + b'x', b'x' + W + b'x']
    for n in ENTRY_LENS:                    # every entry length as an exact fit of one segment of classes around a literal
        if n:
            lines.append(b'T' + b't' * (n - 1))
            patterns += [b'T' + b'?' * (n - 1), b'T' + b'[!x]' * (n - 1) + b'?', b'*T' + b'?' * (n - 1)]
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    r, ref, data = one_chunk(lines)
    try:
        res = check(r, ref, patterns)
        assert (res.counts > 0).sum() > len(patterns) * 3 // 4
    finally:
        r.close()


# ---- 6. chunk edges ----------------------------------------------------------------------------------------------------

def test_chunk_edges_handed_over_on_the_device():
    texts = [b'ab\nxx\nab', b'b', b'q\x00\nqa\nzq', b'a', b'\n', b'cd\nc', b'ab\n\nb?\n']
    r, ref = device_reader(texts), GlobClassRef(texts)
    patterns = [b'a?', b'*a?', b'b?', b'*b?*', b'q[\x00a]', b'*q[\x00a]*', b'q[!x]', b'a[!x]*', b'?b', b'*?b', b'a*?', b'*a', b'c?', b'c[a-z]*',
                b'*[!a]q', b'\\b\\?', b'?*b*']
    try:
        res = per_pattern(check(r, ref, patterns))
        assert sorted(res[0].tolist()) == [0, 2, 6 << 32] and res[2].tolist() == [(6 << 32) | 2]          # `?` takes the last byte; b? not the padding
        assert sorted(res[4].tolist()) == [2 << 32, (2 << 32) | 1] and sorted(res[6].tolist()) == [2 << 32, (2 << 32) | 1]        # a real 0x00, not the padding
        # a literal newline voids its group, and cores that never share a chunk leave nothing to look at
        for fold in (False, True):
            for batch in ([b'a\nb?', b'a?*\n'], [b'*a[a-c]*c[!x]*', b'*q?*d?*']):
                got = r.search_glob_ids_batch(batch, classes=True, icase=fold)
                assert got.ids.size == 0 and r.last_stats()['hits'] == 0
        check(r, ref, [b'a\nb?', b'*a[a-c]*c[!x]*', b'a?'])
    finally:
        r.close()


# ---- 7. fold -----------------------------------------------------------------------------------------------------------

def test_fold(search_env):
    rng = np.random.default_rng(187)
    lines = [b'xBy', b'xby', b'xdy', b'xAy', b'xay', b'xQy', b'K\xc1z', b'k\xe1z', b'k\xc1Z', b'Error: Disk 7', b'ERROR: DISK 9', b'error: disc 7']
    lines += [b'the quick ' + filler(rng, int(rng.integers(0, 9))).upper() for _ in range(40)] + [b'THE SLOW', b'zq The', b'the ZQ']
    r, ref, data = one_chunk(lines)
    patterns = [b'x[a-c]y', b'x[!a]y', b'k\xc1?', b'*error: dis[kc] [0-9]', b'*th[a-e]*z[p-r]*', b'*z[p-r]*th[a-e]*', b'*TH?*', b'x[A-C]y', b'x[!A-Z]y']
    try:
        for letters in (None, 1):
            search_env(PSS_ICASE_SEED_LETTERS=letters)
            H.check(CLASS_ICASE, r, ref, patterns)
        got = per_pattern(r.search_glob_ids_batch(patterns, classes=True, icase=True))
        assert texts_of(r, got[0]) == [b'xAy', b'xBy', b'xay', b'xby'] and texts_of(r, got[1]) == [b'xBy', b'xQy', b'xby', b'xdy']
        assert texts_of(r, got[2]) == [b'K\xc1z', b'k\xc1Z'] and len(got[3]) == 3 and texts_of(r, got[8]) == []
        exact = per_pattern(H.check(CLASS, r, ref, patterns))
        assert texts_of(r, exact[0]) == [b'xay', b'xby'] and texts_of(r, exact[1]) == [b'xAy', b'xBy', b'xQy', b'xby', b'xdy']
        # the driver follows the seed hits: `z` is rarer than `th` whichever comes first
        zq = ref.core_hits(0, b'z', True)
        assert 0 < zq < ref.core_hits(0, b'th', True)
        for p in patterns[4:6]:
            r.count_glob_bytes([p], classes=True, icase=True)
            assert r.last_stats()['hits'] == zq
    finally:
        search_env(PSS_ICASE_SEED_LETTERS=None)
        r.close()


# ---- 8. work and order ---------------------------------------------------------------------------------------------------

def test_hits_follow_the_rarest_core_and_the_order_is_its_candidates():
    rng = np.random.default_rng(188)
    lines = [b'the ' + filler(rng, int(rng.integers(0, 20))) for _ in range(500)]
    lines += [b'the zq9 end', b'zq1 the', b'x the zqa', b'tie uv wx', b'wx uv tie', b'uv', b'wx']
    lines = [lines[int(i)] for i in rng.permutation(len(lines))]
    r, ref, data = one_chunk(lines)
    freq, rare = occurrences(data, b'the'), occurrences(data, b'zq')
    assert freq >= 500 and rare == 3 and occurrences(data, b'uv') == occurrences(data, b'wx') == 3
    try:
        for p in (b'*th[a-e]*zq[0-9]*', b'*zq[0-9]*th[a-e]*', b'*?he*[!a]zq?*', b'???*zq?*'):
            check(r, ref, [p])
            assert r.last_stats()['hits'] == rare, p                     # wherever the rare core stands
        check(r, ref, [b'*th[a-e] *'])
        assert r.last_stats()['hits'] == freq
        check(r, ref, [b'*uv?*wx*', b'*wx?*uv*'])                        # a tie: the lowest index drives
        assert r.last_stats()['hits'] == 6
        batch = [b'*th[a-e]*zq[0-9]*', b'*zq?*', b'*uv?*wx*', b'*wx?*uv*', b'*t?e [a-p]*', b'*?he*', b'the ??*']
        for fold in (False, True):
            got = per_pattern(r.search_glob_ids_batch(batch, classes=True, icase=fold))
            rows = per_pattern(r.search_all_ids_batch([[c[1] for c in glob_cores(p) if c] for p in batch], icase=fold))
            for ids, row, p in zip(got, rows, batch):
                at = {int(v): i for i, v in enumerate(row.tolist())}
                where = [at[int(v)] for v in ids.tolist()]               # (KeyError: an id the cores' row does not hold)
                assert where == sorted(where) and ids.size > 0, p
    finally:
        r.close()


def test_more_candidates_than_the_mid_pipeline_holds():
    rng = np.random.default_rng(189)
    k = 70000
    raw = np.full((k, 4), 0x0A, dtype=np.uint8)
    raw[:, 0] = ord('a')
    raw[:, 1] = rng.integers(ord('0'), ord('4'), k)
    raw[:, 2] = np.where(rng.integers(0, 2, k).astype(bool), ord('x'), ord('y'))
    data = raw.tobytes()
    r, ref = device_reader([data]), GlobClassRef([data])
    try:
        res = per_pattern(check(r, ref, [b'a[0-1]x', b'a?y*', b'*a[!0]?'], texts=False))
        assert r.last_stats()['hits'] == 3 * k > 3 * 65536
        assert res[0].size > k // 8 and res[1].size > k // 3 and res[2].size > k // 2
    finally:
        r.close()


# ---- 9. placement and routes -----------------------------------------------------------------------------------------------

def test_placement(tmp_path, search_env):
    rng = np.random.default_rng(190)
    lines = [b'HEAD%03d ' % i + filler(rng, 6) if i % 40 == 0 else filler(rng, int(rng.integers(0, 24))) for i in range(1500)]
    data = b'\n'.join(lines) + b'\n'
    p = make_index(tmp_path, 'place', data, 4000)
    ref = GlobClassRef.from_index(p)
    assert len(ref.chunks) >= 5
    patterns = [b'*a?b*', b'*b[a-d]a*', b'a*?b', b'HEAD?[0-4]? *', b'*HEAD*a?*b*', b'*p[!p]*', b'*ab*??*cd*', b'*MISS?*a*', b'e?*', b'*?e', b'HEAD*??',
                b'*[!a-p]*a*']
    patterns += [glob_escape(ch.entry(0)[:2], classes=True) + b'?' * (len(ch.entry(0)) - 2) for ch in ref.chunks if len(ch.entry(0)) > 2]
    for fold, kind in ((False, CLASS), (True, CLASS_ICASE)):
        assert H.placement(kind, p, patterns, search_env, ref=ref).ids.size > 100


@pytest.mark.parametrize('route,env', [('INTERVAL_GROUP', {}), ('INTERVAL_LANE', {'PSS_LANE_SEARCH_MIN': 1}),
                                       ('INTERVAL_WAVE', {'PSS_WAVE_SEARCH': 1})])
def test_interval_routes(search_env, route, env):
    """2 400 patterns of one or two cored segments on one chunk (more than 2 048 core pairs) take the 16-lane interval
    search; the switches force the other two."""
    rng = np.random.default_rng(191)
    lines = [filler(rng, int(rng.integers(0, 10))) for _ in range(600)]
    r, ref, data = one_chunk(lines)
    search_env(**env)
    patterns = []
    while len(patterns) < 2400:
        ln = lines[int(rng.integers(0, len(lines)))]
        if len(ln) < 5:
            continue
        cut = int(rng.integers(2, len(ln) - 2))
        a, b = ln[:cut], ln[cut:]
        a = a[:1] + b'?' + a[2:] if len(patterns) % 2 else a[:-1] + b'[a-p]'
        patterns.append((b'', b'*')[int(rng.integers(0, 2))] + a + b'*' + b + (b'', b'*')[int(rng.integers(0, 2))])
    ncores = sum(c is not None for p in patterns for c in glob_cores(p))
    assert 2048 <= ncores < 8192
    try:
        res = H.check(CLASS, r, ref, patterns, interval=R[route])
        assert res.ids.size > 1000
        H.check(CLASS_ICASE, r, ref, patterns[:300])
    finally:
        search_env(**{k: None for k in env})
        r.close()


# ---- 10. errors and conveniences ---------------------------------------------------------------------------------------------

def test_errors():
    rng = np.random.default_rng(192)
    r, ref, data = one_chunk([filler(rng, int(rng.integers(0, 10))) for _ in range(200)] + [b'ab', b'a1b'])
    try:
        for call in (r.search_glob_batch_packed, r.search_glob_ids_batch, r.count_glob_bytes):
            for bad, what in (([b'a?', b'??'], 'nothing in the suffix array'), ([b'a[b'], 'not closed'), ([b'a[z-a]'], 'descends'),
                              ([b'a[\n]'], 'empty'), ([b'a\\'], 'lone backslash')):
                for fold in (False, True):
                    with pytest.raises(ValueError, match=what):
                        call(bad, classes=True, icase=fold)
            with pytest.raises(TypeError):
                call(b'a?b', classes=True)
        h = r._handle()
        for what, (args, keep) in BAD_C_BATCHES:            # through the C ABI: PSS_EINVAL with a message, *out and counts untouched
            for fn in (_ffi.lib.pss_reader_search_seqc_batch, _ffi.lib.pss_reader_search_seqc_ids_batch):
                out = ctypes.c_void_p()
                assert fn(h, *args, ctypes.byref(out)) == _ffi.PSS_EINVAL
                assert not out.value and what in _ffi.last_error(), (what, _ffi.last_error())
            counts = np.full(4, 7, dtype=np.uint64)
            assert _ffi.lib.pss_reader_count_seqc_batch(h, *args, counts.ctypes.data) == _ffi.PSS_EINVAL
            assert counts.tolist() == [7] * 4 and what in _ffi.last_error()
        args, keep = c_args([b'a\0b'], [b'\0\1\0'], [b'0123456789'], [0, 1], [3])
        assert _ffi.lib.pss_reader_search_seqc_batch(h, *args, None) == _ffi.PSS_EINVAL
        assert _ffi.lib.pss_reader_count_seqc_batch(h, *args, None) == _ffi.PSS_EINVAL
        out = ctypes.c_void_p()                             # ... and the good batch goes through the same call; the reader still answers
        assert _ffi.lib.pss_reader_search_seqc_batch(h, *args, ctypes.byref(out)) == _ffi.PSS_OK and out.value
        assert _ffi.lib.pss_result_num_entries(out) == 1
        _ffi.lib.pss_result_free(out)
        check(r, ref, [b'a?b', b'*a[0-9]*'])
        H.check(H.GLOB, r, GlobRef([data]), [b'*a*b*', b'a?b', b'a1b'])          # (without the keyword: `?` is a byte)
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
        one = ['some short string']
        assert r.search_glob('some?short*', classes=True) == r.search_glob('*sh[a-o]rt*', classes=True) == r.search_glob('s???*g', classes=True) == one
        assert r.search_glob('SOME?SHORT*', classes=True, icase=True) == r.search_glob('*[!x]tring', classes=True) == one
        assert r.search_glob('some?short', classes=True) == [] and r.search_glob('*sh[!o]rt*', classes=True) == [] and r.search_glob('SOME*', classes=True) == []
        assert r.search_glob('some?short*') == [] and r.search_glob('some short string?', classes=True) == []
        assert r.count_glob('*s?r*', classes=True) == 1 and r.count_glob('*S?R*', classes=True, icase=True) == 1 and r.count_glob('*s?r', classes=True) == 0
        for bad in (b'some?', ['some?'], None):
            with pytest.raises(TypeError):
                r.search_glob(bad, classes=True)
        for bad in ('', '*', '??', '*[a-z]*', 'some[', 'some\\'):
            with pytest.raises(ValueError):
                r.search_glob(bad, classes=True)
            with pytest.raises(ValueError):
                r.count_glob(bad, classes=True, icase=True)
        with pytest.raises(TypeError):
            r.search_glob('some*', classes='yes')
    finally:
        r.close()


@pytest.mark.parametrize('kind', [CLASS, CLASS_ICASE], ids=lambda kind: kind.name)
def test_rows_and_core_bytes_around_a_multiple_of_64(kind):
    """63, 64 and 65 patterns whose core bytes add up to 31, 32 and 33 modulo 64 -- a class position behind the first core --, on one
    chunk and on three (search_harness.layout_edges)."""
    H.layout_edges(kind, lambda groups: H.edge_globs(groups, gap=b'?*'), min_ids=63)
