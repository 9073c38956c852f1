"""Every route of the Reader's search against a brute-force reference (tests/search_ref.py), at the edges where it
changes behaviour: comparison edges (query lengths around the 8-byte words, 0x00 / 0x7F / 0x80 / 0xFF at word edges,
the zero padding past the text), the key-sample window, the batch-size thresholds between the fused kernels, the
interval kernels and the pipelines, the capacities of the fused path, the per-entry dedupe, the suffix-array result
order and the host tier.  Inputs are built so that a marker query occurs only where it was placed (the filler never
uses its bytes).  Every case compares per-query counts and multisets through search_batch_raw, search_batch_packed,
count_multiple_bytes and the single-query path (low-latency mode on and off), and asserts last_stats()['route'], so
that it proves it reached the branch it names.  The last test checks that the module saw every PSS_ROUTE_* bit."""
import os
import pathlib
import re

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests.search_harness import FUSED, SEEN, filler, finished, make_index
from tests.search_ref import SearchRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = _ffi.ROUTES
SM_MAX_HITS = 1024              # hits of one pair that the wave kernel takes (search.hip); the block path takes 1024 per workgroup


def expect_route(rt, want, what=''):
    """rt shows every bit of `want`; a fused kernel or the mid pipeline named without its overflow bit must have
    finished the batch itself (the bit of a route is set when it starts, its overflow bit when it gives up)."""
    assert rt & want == want, (what, hex(rt), hex(want))
    if want & FUSED and not want & R['SMALL_OVERFLOW']:
        assert not rt & R['SMALL_OVERFLOW'], (what, 'the fused kernel overflowed', hex(rt))
    if want & R['MID'] and not want & R['MID_OVERFLOW']:
        assert not rt & R['MID_OVERFLOW'], (what, 'the mid pipeline overflowed', hex(rt))


class Case:
    """One index: the reader, the reference, and a memo of the reference's answers."""

    def __init__(self, path, **reader_kw):
        self.path = path
        self.ref = SearchRef.from_index(path)
        self.memo = {}
        self.r = pysubstringsearch.Reader(path, **reader_kw)

    def close(self):
        self.r.close()

    def want(self, q):
        if q not in self.memo:
            self.memo[q] = sorted(self.ref.search(q))
        return self.memo[q]

    def route(self):
        rt = self.r.last_stats()['route']
        SEEN[0] |= finished(rt)
        return rt

    @staticmethod
    def pad(queries, n):
        """queries and misses (bytes no index here holds) up to n of them: more pairs, no more entries."""
        return list(queries) + [b'\x01MISS' + i.to_bytes(2, 'little') for i in range(n - len(queries))]

    def split(self, queries, cap=SM_MAX_HITS):
        """(queries with at most `cap` hits in every chunk, the others): a wave-kernel batch of the first finishes on
        the fused path; the second overflows it."""
        light = [q for q in queries if max(self.ref.hits(q)) <= cap]
        return light, [q for q in queries if q not in light]

    def batch(self, queries, route=0, single=16, packed=True, counts=True):
        """queries through every path; `route`: bits the raw batch must show.  Returns the raw batch's route."""
        ents, counts_got = self.r.search_batch_raw(queries)
        rt = self.route()
        want = [self.want(q) for q in queries]
        assert counts_got == [len(w) for w in want], [(q[:12], c, len(w)) for q, c, w in zip(queries, counts_got, want)
                                                       if c != len(w)][:4]
        pos = 0
        for q, w in zip(queries, want):
            assert sorted(ents[pos:pos + len(w)]) == w, q[:40]
            pos += len(w)
        expect_route(rt, route, 'batch')
        if packed:
            pk = self.r.search_batch_packed(queries)
            self.route()
            assert pk.counts.tolist() == counts_got
            blob = pk.data.tobytes()
            off = pk.offsets.tolist()
            got = [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]
            pos = 0
            for w in want:
                assert sorted(got[pos:pos + len(w)]) == w
                pos += len(w)
        if counts:
            assert self.r.count_multiple_bytes(queries) == counts_got
            assert self.route() & (R['COUNTS'] | R['GENERAL']) == R['COUNTS'] | R['GENERAL']
        if single:
            self.singles(queries[:single // 2] + queries[-(single // 2):])
        return rt

    def singles(self, queries, route_on=0, route_off=0):
        """One query per call, low-latency mode on (route_on) and off (route_off).  The resident kernel may decline a
        query (the launch path answers it then): RESIDENT is required of one query of the call, other bits of each."""
        for on in (True, False):
            self.r.set_low_latency(on)
            want = route_on if on else route_off
            seen = 0
            for q in queries:
                ents, c = self.r.search_batch_raw([q])
                rt = self.route()
                seen |= rt
                assert c == [len(self.want(q))] and sorted(ents) == self.want(q), (on, q[:40])
                expect_route(rt, want & ~R['RESIDENT'], (on, q[:40]))
            assert seen & want == want, (on, hex(seen))
        self.r.set_low_latency(False)


# ------------------------------------------------------------------------------------------------ comparison edges --

def comparison_text(rng):
    """Lines of filler with markers at every alignment, a long unique line, '\\n'-adjacent markers, 0x00 .. 0xFF."""
    lines = []
    for b in (0x00, 0x7F, 0x80, 0xFF):
        for off in range(9):
            head = filler(rng, off)
            # the byte as the first and as the last byte of an 8-byte word of the query (and of the text at every shift)
            lines.append(head + bytes([b]) + b'QRSTUVW' + bytes([b]) + b'XYZ' + filler(rng, 5))
            lines.append(head + b'QRSTUVW' + bytes([b]) + bytes([b]) + b'QRSTUVW' + filler(rng, 3))
    lines.append(bytes(rng.integers(0x11, 0x60, 1200, dtype=np.uint8)).replace(b'\n', b'_'))   # the long unique line
    lines += [b'', b'', b'ZZ', b'ZZ\x00', b'\x00', b'\xff\xff', b'ZZ' + filler(rng, 20)]
    lines.append(b'KEYS0123' + b'A' + filler(rng, 4))
    lines.append(b'KEYS0123' + b'B' + filler(rng, 4))
    lines.append(b'KEYS0123')
    for k in range(40):
        lines.append(filler(rng, int(rng.integers(0, 30))))
    lines.append(b'TAILTAIL\x01\x02\x03')          # the last entry: its bytes end the chunk (then its '\n')
    return b'\n'.join(lines) + b'\n'


def comparison_queries(data):
    long_line = max(data.split(b'\n'), key=len)
    qs = [b'', b'\n', b'\n\n', b'ZZ\n', b'\nZZ', b'ZZ\n\x00', b'\x00\n', b'\xff', b'\xff\xff\n', b'\x00' * 8]
    for L in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000):
        qs.append(long_line[:L])
        qs.append(long_line[100:100 + L])
        qs.append(long_line[:L - 1] + b'\x7e')                # differs at the last byte: no hit
    for b in (0x00, 0x7F, 0x80, 0xFF):
        c = bytes([b])
        qs += [c + b'QRSTUVW', c + b'QRSTUVW' + c, b'QRSTUVW' + c, b'QRSTUVW' + c + c, b'W' + c + c + b'Q',
               c + b'QRSTUVW' + c + b'XYZ', b'QRSTUVW' + c + c + b'QRSTUVW', c, c + c]
    qs += [b'KEYS0123', b'KEYS0123A', b'KEYS0123C', b'KEYS0123\n', b'KEYS012', b'KEYS0123\x00']
    # the end of the chunk: a proper prefix of the last suffixes, and queries that run past the text into its padding
    qs += [b'TAILTAIL\x01\x02', b'TAILTAIL\x01\x02\x03', b'TAILTAIL\x01\x02\x03\n', b'TAILTAIL\x01\x02\x03\n\x00',
           b'\x03\n\x00', b'\n\x00', b'\x02\x03\n\x00\x00\x00\x00\x00\x00\x00']
    return qs


# (switches, route of the batch of short queries, route of each single short query without low latency)
COMPARISON_ROUTES = [
    ({}, R['SMALL_WAVE'], R['SMALL_BLOCK']),
    ({'PSS_NO_BLOCK_PATH': 1}, R['SMALL_WAVE'], R['SMALL_WAVE']),
    ({'PSS_NO_SMALL_PATH': 1}, R['INTERVAL_WAVE'] | R['MID'], R['INTERVAL_WAVE'] | R['MID']),
    ({'PSS_NO_SMALL_PATH': 1, 'PSS_LANE_SEARCH_MIN': 1}, R['INTERVAL_LANE'] | R['MID'], R['INTERVAL_LANE'] | R['MID']),
    ({'PSS_NO_SMALL_PATH': 1, 'PSS_WAVE_SEARCH': 1, 'PSS_NO_MID_PIPELINE': 1}, R['INTERVAL_WAVE'] | R['GENERAL'], 0),
    ({'PSS_NO_SMALL_PATH': 1, 'PSS_NO_SEARCH_STAGE': 1}, R['INTERVAL_WAVE'] | R['MID'], 0),
]
SWITCHES_OFF = {k: None for e, _, _ in COMPARISON_ROUTES for k in e}


@pytest.mark.parametrize('samples', [None, 0, 1, 5, 11, 'off'])
def test_comparison_edges(tmp_path, search_env, samples):
    rng = np.random.default_rng(1)
    data = comparison_text(rng)
    p = make_index(tmp_path, 'cmp', data)
    search_env(PSS_NO_KEY_SAMPLES=1 if samples == 'off' else None,
               PSS_SAMPLE_SHIFT=None if samples in (None, 'off') else samples)
    c = Case(p)
    try:
        qs = comparison_queries(data)
        short = [q for q in qs if len(q) <= 256]            # the fused kernels take queries of up to 256 bytes
        assert 65 <= len(short) <= 1023 and sum(map(len, qs)) < 8000
        ks = 0 if samples == 'off' else R['KEY_SAMPLES']
        light, heavy = c.split(short)
        assert len(light) >= 65 and heavy == [b'']             # the empty query: a hit at every byte of the text
        for env, route, single_route in COMPARISON_ROUTES:
            search_env(**SWITCHES_OFF)
            search_env(**env)
            rt = c.batch(light, route | ks, single=0)
            assert samples != 'off' or not rt & R['KEY_SAMPLES']
            if route & FUSED:
                c.batch(heavy + light, route | R['SMALL_OVERFLOW'] | ks, single=0, packed=False, counts=False)
            c.singles(light if not env else light[::7], route_on=R['RESIDENT'] if not env else 0, route_off=single_route)
            c.singles(heavy, route_off=single_route if single_route != R['SMALL_WAVE'] else 0)
        search_env(**SWITCHES_OFF)
        c.batch(qs, R['INTERVAL_WAVE'] | R['MID'] | ks, single=0)      # queries longer than 256 bytes: no fused kernel
        c.singles([q for q in qs if len(q) > 256], route_off=R['INTERVAL_WAVE'] | R['MID'])
        # the 16-lane interval kernel needs >= 2048 pairs
        many = [q for q in qs if q not in heavy]               # 2100 pairs whose hits stay within the mid pipeline
        big = (many * (2100 // len(many) + 1))[:2100]
        c.batch(big, R['INTERVAL_GROUP'] | R['MID'] | ks, single=0, packed=False)
        search_env(PSS_NO_GROUP_SEARCH=1)
        c.batch(big, R['INTERVAL_WAVE'] | R['MID'] | ks, single=0, packed=False, counts=False)
    finally:
        c.close()


# -------------------------------------------------------------------------------------------- key-sample window --

@pytest.mark.parametrize('shift', [0, 1, 5, 11])
def test_key_sample_window(tmp_path, search_env, shift):
    rng = np.random.default_rng(2 + shift)
    step = 1 << shift
    k = max(3, (4096 >> shift) if shift < 11 else 70)
    lengths = [k * step - 1, k * step, k * step + 1]
    if shift >= 5:
        lengths.append(step - 1)                   # a chunk shorter than one sample step
    run = 65 * step + 64                           # > 64 samples share the 8-byte prefix 'PPPPPPPP'
    search_env(PSS_SAMPLE_SHIFT=shift)
    for n in lengths:
        body = b'\x00\x00X\n~~\xff\xfe\n'
        if n > run + 400:
            body += filler(rng, 40) + b'\n' + b'P' * run + b'Q\n'
        tail = n - len(body) - 1
        assert tail >= 0
        data = body + filler(rng, tail).replace(b'p', b'\n') + b'\n'
        assert len(data) == n
        c = Case(make_index(tmp_path, f'k{n}', data))
        try:
            assert c.ref.chunks[0].text == data
            qs = [b'', b'\x00', b'\x00\x00', b'\x00\x00X\n', b'\x00\x01', b'\xff', b'\xff\xff\xff', b'~', b'~~\xff\xfe',
                  b'~~\xff\xff', b'\xfe\n', b'PPPPPPPP', b'PPPPPPPPQ', b'PPPPPPPPR', b'PPPP', b'PQ', b'P' * 9 + b'Q',
                  b'a', b'ab', b'abc', b'\na', b'a\n', data[-9:], data[-3:], data[-2:] + b'\x00']
            qs += [data[i:i + 1 + i % 13] for i in range(5, n - 1, max(1, n // 40))]
            qs = qs[:64]
            ks = R['KEY_SAMPLES']
            light, heavy = c.split(qs)
            assert len(light) >= 20
            c.batch(light, ks | R['SMALL_BLOCK'], single=0, packed=False, counts=False)
            c.singles(light, route_off=R['SMALL_BLOCK'])
            c.batch(c.pad(light, 100), ks | R['SMALL_WAVE'], single=0)
            if heavy:
                c.batch(c.pad(heavy + light, 100), ks | R['SMALL_WAVE'] | R['SMALL_OVERFLOW'], single=0, counts=False)
            for env, route in (({'PSS_WAVE_SEARCH': 1}, R['INTERVAL_WAVE']),
                               ({'PSS_LANE_SEARCH_MIN': 1}, R['INTERVAL_LANE'])):
                search_env(PSS_NO_SMALL_PATH=1, **env)
                c.batch(qs, ks | route, single=0, packed=False)
                search_env(PSS_NO_SMALL_PATH=None, **{e: None for e in env})
            big = (qs * (2048 // len(qs) + 1))[:2048]
            c.batch(big, ks | R['INTERVAL_GROUP'], single=0, packed=False, counts=False)
            search_env(PSS_NO_GROUP_SEARCH=1)
            c.batch(big, ks | R['INTERVAL_WAVE'], single=0, packed=False, counts=False)
            search_env(PSS_NO_GROUP_SEARCH=None)
        finally:
            c.close()


# ---------------------------------------------------------------------------------------------- batch thresholds --

def threshold_text(rng, n_lines):
    lines = [filler(rng, int(rng.integers(0, 24))) for _ in range(n_lines)]
    return b'\n'.join(lines) + b'\n'


def threshold_queries(rng, data, nq):
    qs = []
    for i in range(nq):
        if i % 5 == 4:
            qs.append(b'MISS' + i.to_bytes(4, 'little'))
        else:
            s = int(rng.integers(0, len(data) - 8))
            qs.append(data[s:s + 6 + i % 4])           # about one hit each: 65 536 pairs stay within the mid pipeline
    return qs


def expected_route(queries, nc):
    """The route search_batch_device picks for a batch (search.hip), before any overflow."""
    nq, nvq = len(queries), len(queries) * nc
    tiny = sum(map(len, queries)) + 32 <= 8192 and (nq + 1) * 8 <= 8192
    if tiny and nvq <= 1024 and max(map(len, queries)) <= 256:
        return R['SMALL_BLOCK'] if nvq <= 64 else R['SMALL_WAVE']
    rt = R['INTERVAL_LANE'] if nvq >= 8192 else R['INTERVAL_GROUP'] if nvq >= 2048 else R['INTERVAL_WAVE']
    return rt | (R['MID'] if nvq <= 65536 else R['GENERAL'])


@pytest.mark.parametrize('chunks', [1, 5])
def test_batch_size_thresholds(tmp_path, search_env, chunks):
    """(query, chunk) pairs at 1, 64 / 65, 1024 / 1025, 2047 / 2048, 8191 / 8192 and 65 536 / 65 537 (on several chunks:
    the nearest multiples on both sides), nq = 1023 / 1024 and query bytes of 8 KiB - 32 +- 1 at the 8 KiB staging, a
    batch over the 2 MiB query staging, and the switches of the staging, the block path, the mid pipeline and the
    pinned results."""
    rng = np.random.default_rng(3)
    data = threshold_text(rng, 6000)
    p = make_index(tmp_path, 'th', data, None if chunks == 1 else len(data) // chunks + 200)
    c = Case(p)
    try:
        nc = c.r.num_chunks
        assert (nc == 1) == (chunks == 1)
        ks = R['KEY_SAMPLES']
        for nvq in (1, 64, 65, 1024, 1025, 2047, 2048, 8191, 8192, 65536, 65537):
            for nq in sorted({max(1, nvq // nc), max(1, -(-nvq // nc))}):
                qs = threshold_queries(rng, data, nq)
                c.batch(qs, expected_route(qs, nc) | ks, single=4 if nq < 2000 else 0, packed=nq < 20000)
        for nq in (1023, 1024):                 # the offsets of 1024 queries do not fit the 8 KiB staging
            qs = threshold_queries(rng, data, nq)
            rt = c.batch(qs, expected_route(qs, nc) | ks, single=0, packed=False, counts=False)
            assert bool(rt & R['SMALL_WAVE']) == (nq == 1023 and nc == 1), hex(rt)
        for total in (8160, 8161):              # query bytes + 32 against the 8 KiB staging
            qs = [data[i * 40:i * 40 + 40] for i in range(total // 40 - 1)] + [data[7000:7000 + 40 + total % 40]]
            assert sum(map(len, qs)) == total
            rt = c.batch(qs, expected_route(qs, nc) | ks, single=0, packed=False, counts=False)
            assert bool(rt & (R['SMALL_WAVE'] | R['SMALL_BLOCK'])) == (total == 8160 and len(qs) * nc <= 1024), hex(rt)
        long_qs = [data[s:s + 2100] for s in range(0, 1001 * 7, 7)]     # over the 2 MiB pinned query staging
        assert sum(map(len, long_qs)) + 8 * (len(long_qs) + 1) + 96 > 2 << 20
        c.batch(long_qs, expected_route(long_qs, nc) | ks, single=0, packed=False)
        qs = threshold_queries(rng, data, 3000)
        for env in ({'PSS_NO_SEARCH_STAGE': 1}, {'PSS_NO_BLOCK_PATH': 1}, {'PSS_NO_MID_PIPELINE': 1},
                    {'PSS_NO_PINNED_RESULTS': 1}):
            search_env(**env)
            want = expected_route(qs, nc)
            if 'PSS_NO_MID_PIPELINE' in env:
                want = (want & ~R['MID']) | R['GENERAL']
            c.batch(qs, want | ks, single=4, packed=False)
            c.batch(qs[:150], R['SMALL_WAVE'] | ks, single=0, packed=False, counts=False)
            c.singles(qs[:3], route_off=R['SMALL_WAVE'] if 'PSS_NO_BLOCK_PATH' in env else R['SMALL_BLOCK'])
            search_env(**{k: None for k in env})
    finally:
        c.close()


# -------------------------------------------------------------------------------------------- fused capacities --

def marker_lines(rng, marker, n, width=6):
    return [filler(rng, int(rng.integers(0, width))) + marker + filler(rng, int(rng.integers(0, width))) for _ in range(n)]


def test_fused_hit_capacities(tmp_path, search_env):
    """One pair with 1023 / 1024 / 1025 hits (hash dedupe against the spread path's hit_entry) and 32 768 / 32 769 hits
    (SM_SPREAD x 1024: the second overflows the fused path)."""
    rng = np.random.default_rng(4)
    lines = []
    for n, m in ((1023, b'Q3'), (1024, b'Q4'), (1025, b'Q5'), (32768, b'R8'), (32769, b'R9')):
        lines += marker_lines(rng, m, n)
    # periodic queries in runs: 1024 / 1025 hits inside ONE entry
    lines += [b'W' + b'ST' * 1025 + b'W', b'V' * 1026, b'U' * 1027]
    order = rng.permutation(len(lines))
    data = b'\n'.join(lines[i] for i in order) + b'\n'
    c = Case(make_index(tmp_path, 'cap', data))
    try:
        small = R['SMALL_BLOCK']
        for q, n in ((b'Q3', 1023), (b'Q4', 1024), (b'Q5', 1025), (b'R8', 32768)):
            assert len(c.want(q)) == n
            c.singles([q], route_on=small if n > 1024 else R['RESIDENT'], route_off=small)
            rt = c.batch([q], small, single=0)
            assert not rt & R['SMALL_OVERFLOW']
        c.singles([b'R9'], route_on=small | R['SMALL_OVERFLOW'], route_off=small | R['SMALL_OVERFLOW'] | R['MID'])
        c.batch([b'R9'], small | R['SMALL_OVERFLOW'] | R['MID'], single=0)
        for q in (b'STST', b'TSTS', b'VVV', b'UUU', b'VV', b'UU', b'ST' * 30, b'V' * 200):
            assert len(c.want(q)) == 1
        c.singles([b'STS', b'VVV', b'UUU', b'UU', b'STST'], route_off=small)
        c.batch([b'STS', b'VVV', b'UUU', b'UU', b'STST', b'ST' * 30], small, single=0)
        c.batch(c.pad([b'STS', b'VVV', b'STST', b'ST' * 30, b'TSTS'], 65), R['SMALL_WAVE'], single=0)   # <= 1024 hits
        c.batch(c.pad([b'UUU', b'UU', b'STS'], 65), R['SMALL_WAVE'] | R['SMALL_OVERFLOW'], single=0)
    finally:
        c.close()


@pytest.mark.parametrize('n_chunks', [32, 33, 64, 65])
def test_one_query_over_many_chunks(tmp_path, n_chunks):
    """One query over 32 chunks (2 workgroups per pair), 33 .. 64 chunks (4 workgroups per pair): a chunk with 2000 hits
    stays on the fused path; more than 64 chunks: one wavefront per pair, which takes at most 1024 hits."""
    rng = np.random.default_rng(5)
    p = str(tmp_path / 'many.idx')
    w = pysubstringsearch.Writer(p)
    for k in range(n_chunks):
        for line in marker_lines(rng, b'MK', 2000 if k == 7 else int(rng.integers(0, 20)), 3):
            w.add_entry(line.decode())
        for _ in range(30):
            w.add_entry(filler(rng, 30).decode())
        w.dump_data()
    w.close()
    c = Case(p)
    try:
        assert c.r.num_chunks == n_chunks
        assert len(c.want(b'MK')) > 2000
        if n_chunks <= 64:
            rt = c.batch([b'MK'], R['SMALL_BLOCK'], single=0)
            assert not rt & R['SMALL_OVERFLOW']
            c.singles([b'MK', b'MKa', b'aMK'], route_off=R['SMALL_BLOCK'])
        else:
            c.batch([b'MK'], R['SMALL_WAVE'] | R['SMALL_OVERFLOW'] | R['MID'], single=0)
            rt = c.batch([b'MKa', b'aMK'], R['SMALL_WAVE'], single=0)
            assert not rt & R['SMALL_OVERFLOW']
            c.singles([b'MKa'], route_off=R['SMALL_WAVE'])
            c.singles([b'MK'], route_off=R['SMALL_WAVE'] | R['SMALL_OVERFLOW'])
    finally:
        c.close()


def test_entry_capacity_of_the_wave_kernel(tmp_path):
    """65 535 / 65 536 / 65 537 entries in one batch of 65 pairs on search_small_kernel (SM_ENT_CAP = 65 536)."""
    rng = np.random.default_rng(6)
    markers = [bytes([0x41 + i // 26, 0x41 + i % 26]) + b'#' for i in range(66)]
    lines = []
    for i, m in enumerate(markers):
        lines += marker_lines(rng, m, 1024 if i < 64 else 1 if i == 64 else 1023, 3)
    order = rng.permutation(len(lines))
    data = b'\n'.join(lines[i] for i in order) + b'\n'
    c = Case(make_index(tmp_path, 'ent', data))
    try:
        miss = b'#zz'
        for total, qs in ((65535, markers[:63] + [markers[65], miss]), (65536, markers[:64] + [miss]),
                          (65537, markers[:65])):
            assert len(qs) == 65 and sum(len(c.want(q)) for q in qs) == total
            over = R['SMALL_OVERFLOW'] if total > 65536 else 0
            rt = c.batch(qs, R['SMALL_WAVE'] | over, single=0, packed=total == 65536, counts=False)
            assert rt & R['SMALL_OVERFLOW'] == over, hex(rt)
    finally:
        c.close()


def sized_lines(rng, marker, n, total):
    """n lines holding `marker` once, of total bytes `total` (line bytes, without their '\\n')."""
    base = total // n
    sizes = [base] * n
    for i in range(total - base * n):
        sizes[i] += 1
    out = []
    for s in sizes:
        assert s >= len(marker)
        head = int(rng.integers(0, s - len(marker) + 1))
        out.append(filler(rng, head) + marker + filler(rng, s - len(marker) - head))
    return out


def test_copy_branches_of_the_block_path(tmp_path):
    """Result bytes at the edges of block_pair's copy branches: 512 / 513 bytes with 16 / 17 entries (direct stores of the
    resident kernel), 48 KiB - 16 +- 1 (LDS stage), 64 KiB +- 1 in one workgroup and split over several (pinned prefix
    against the device arena), an entry longer than the stage."""
    rng = np.random.default_rng(7)
    cases = {b'D0': (16, 512), b'D1': (16, 513), b'D2': (17, 512), b'D3': (17, 513),
             b'S0': (200, 48 * 1024 - 17), b'S1': (200, 48 * 1024 - 16), b'S2': (200, 48 * 1024 - 15),
             b'P0': (500, 65535), b'P1': (500, 65536), b'P2': (500, 65537),
             b'X0': (1500, 65535), b'X1': (1500, 65536), b'X2': (1500, 65537),
             b'L0': (1, 60000), b'L1': (3, 50000 * 3)}
    lines = []
    for m, (n, total) in cases.items():
        lines += sized_lines(rng, m, n, total)
    order = rng.permutation(len(lines))
    data = b'\n'.join(lines[i] for i in order) + b'\n'
    c = Case(make_index(tmp_path, 'copy', data))
    try:
        for m, (n, total) in cases.items():
            w = c.want(m)
            assert len(w) == n and sum(map(len, w)) == total, m
            c.singles([m], route_on=R['RESIDENT'] if n <= 1024 else R['SMALL_BLOCK'], route_off=R['SMALL_BLOCK'])
            st = c.r.last_stats()
            assert st['entries'] == n and st['result_bytes'] == total
        c.batch(list(cases), R['SMALL_BLOCK'], single=0)
        light, heavy = c.split(list(cases))
        assert heavy == [b'X0', b'X1', b'X2']
        c.batch(c.pad(light, 70), R['SMALL_WAVE'], single=0)
        c.batch(heavy + light * 6, R['SMALL_WAVE'] | R['SMALL_OVERFLOW'], single=0, counts=False)
    finally:
        c.close()


def test_byte_capacities_of_the_fused_path_and_the_mid_pipeline(tmp_path, search_env):
    """8 MiB (SM_BYTE_CAP) and 16 MiB (the mid pipeline's byte_cap), each exactly and one byte over."""
    rng = np.random.default_rng(8)
    E = 8192
    lines = []
    for i in range(2048):
        mk = b'\xfb' + (b'\xfc' if i < 1024 else b'') + b'\xfe'
        lines.append(filler(rng, E - len(mk) - 3) + mk + filler(rng, 3))
    lines[0] = lines[0][:E - 1] + b'\xfd'                   # \xfd: in 1024 entries of 8 MiB, and one entry more
    for i in range(1, 1024):
        lines[i] = lines[i][:10] + b'\xfd' + lines[i][11:]
    lines.append(b'\xfe')                                 # + 1 byte: 16 MiB + 1 for \xfe
    lines.append(b'\xfd')                                 # + 1 byte: 8 MiB + 1 for \xfd
    order = rng.permutation(len(lines))
    data = b'\n'.join(lines[i] for i in order) + b'\n'
    assert b'\xfb\xfb' not in data
    c = Case(make_index(tmp_path, 'bytes', data))
    try:
        def size(q):
            return sum(map(len, c.want(q)))
        assert size(b'\xfc') == 8 << 20 and size(b'\xfd') == (8 << 20) + 1
        assert size(b'\xfb') == 16 << 20 and size(b'\xfe') == (16 << 20) + 1
        blk = R['SMALL_BLOCK']
        rt = c.batch([b'\xfc'], blk, single=0, packed=False, counts=False)
        assert not rt & R['SMALL_OVERFLOW']
        c.batch([b'\xfd'], blk | R['SMALL_OVERFLOW'] | R['MID'], single=0, packed=False, counts=False)
        rt = c.batch([b'\xfb'], blk | R['SMALL_OVERFLOW'] | R['MID'], single=0, packed=False, counts=False)
        assert not rt & R['MID_OVERFLOW']
        c.batch([b'\xfe'], blk | R['SMALL_OVERFLOW'] | R['MID'] | R['MID_OVERFLOW'] | R['GENERAL'], single=0)
        search_env(PSS_NO_PINNED_RESULTS=1)
        c.batch([b'\xfe', b'\xfd'], R['MID_OVERFLOW'] | R['GENERAL'], single=0, packed=False, counts=False)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------- dedupe --

def dedupe_lines(rng, first, L):
    """One entry per distance d = L .. 140 with the query at p and at p + d (the second occurrence is the duplicate),
    at shifting alignments, and one entry with a single occurrence.  The query is `first` and L - 1 bytes that the
    filler and the other lengths' queries never use."""
    tail = {1: b'', 7: b'ABCDEF', 8: b'GHIJKLM', 9: b'NOPQRSTU', 20: b'#' * 19}[L]
    q = bytes([first]) + tail
    out = []
    for d in range(L, 141):
        head = filler(rng, (d * 3) % 17)
        out.append(head + q + filler(rng, d - L) + q + filler(rng, d % 5))
    out.append(q)
    return q, out


@pytest.mark.parametrize('first', [0x00, 0x09, 0x0B])
def test_earlier_occurrence_at_every_distance(tmp_path, search_env, first):
    """An earlier occurrence of the query at every distance 1 .. 140 before a hit in the same entry: across the 8-byte
    words and 64-byte blocks of hit_entry's backward scan, candidates that straddle two words, query lengths 1, 7, 8,
    9 and 20 -- through the hash dedupe of the block path, hit_entry in the wave kernel (every batch finishes there),
    in the mid pipeline and in the general pipeline."""
    rng = np.random.default_rng(9 + first)
    for L in (1, 7, 8, 9, 20):
        q, lines = dedupe_lines(rng, first, L)
        data = b'\n'.join(lines + [b'', filler(rng, 10)]) + b'\n'
        search_env(PSS_NO_SMALL_PATH=None, PSS_NO_MID_PIPELINE=None)
        c = Case(make_index(tmp_path, f'dd{L}', data))
        try:
            assert len(c.want(q)) == 142 - L and max(c.ref.hits(q)) <= SM_MAX_HITS
            c.singles([q], route_on=R['RESIDENT'], route_off=R['SMALL_BLOCK'])
            c.batch(c.pad([q, q[:1]], 65), R['SMALL_WAVE'], single=0)           # hit_entry in the wave kernel
            search_env(PSS_NO_SMALL_PATH=1)
            c.batch([q, q[:1]], R['MID'], single=0, counts=False)              # hit_entry in hit_lines
            search_env(PSS_NO_MID_PIPELINE=1)
            c.batch([q, q[:1]], R['GENERAL'], single=0, counts=False)
        finally:
            c.close()


def test_earlier_occurrence_in_the_first_bytes_of_a_chunk(tmp_path, search_env):
    """The duplicate inside the first 8 bytes of a chunk, where hit_entry's byte-by-byte tail loop runs."""
    p = str(tmp_path / 'first.idx')
    w = pysubstringsearch.Writer(p)
    qs = []
    for first in ('\x00', '\x09', '\x0b'):
        for L in (1, 2, 3):
            q = (first + 'QR')[:L]
            qs.append(q.encode())
            for d in range(L, 9):
                w.add_entry(q + 'a' * (d - L) + q + 'bcd')
                w.dump_data()
                w.add_entry('ab' * d + q + 'c' * d + q)
                w.dump_data()
    w.close()
    c = Case(p)
    try:
        assert c.r.num_chunks > 50
        c.batch(sorted(set(qs)), 0, single=0)
        c.singles(sorted(set(qs))[:3], route_off=R['SMALL_WAVE'])
        search_env(PSS_NO_SMALL_PATH=1)
        c.batch(sorted(set(qs)), R['MID'], single=0, counts=False)
    finally:
        c.close()


def test_empty_entries_and_empty_query(tmp_path):
    rng = np.random.default_rng(10)
    data = b'\n\n' + filler(rng, 20) + b'\n\n\n' + b'E' * 70000 + b'\n\n' + filler(rng, 3) + b'\n'
    c = Case(make_index(tmp_path, 'empty', data))
    try:
        qs = [b'', b'\n', b'\n\n', b'\n\n\n', b'\n\n\n\n', b'E', b'EE\n', b'\nE']
        c.batch(qs, 0, single=len(qs))
        light, heavy = c.split(qs)
        assert heavy == [b'', b'E']
        c.batch(c.pad(light, 70), R['SMALL_WAVE'], single=0)
        c.batch(qs * 10, R['SMALL_WAVE'] | R['SMALL_OVERFLOW'], single=0)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ orders and tiers --

@pytest.mark.parametrize('chunk_len', [None, 1500])
def test_sa_order_equals_the_oracle_lists(tmp_path, oracle, chunk_len):
    rng = np.random.default_rng(11)
    data = comparison_text(rng) + b'\n'.join(marker_lines(rng, b'ZZ', 40)) + b'\nZZaZZbZZ\n'
    p = make_index(tmp_path, 'sa', data, chunk_len)
    o = oracle.OracleReader(p)
    c = Case(p, order='sa')
    try:
        qs = comparison_queries(data) + [b'ZZ', b'Z', b'a', b'\x00', b'']
        c.batch(qs, R['GENERAL'] | R['SA_ORDER'], single=0)
        ents, counts = c.r.search_batch_raw(qs)
        assert c.route() & R['SA_ORDER']
        oe, oc = o.search_multiple_bytes(qs)
        assert counts == oc.tolist() and ents == oe               # element by element
        for q in qs[:20]:
            assert c.r.search_batch_raw([q])[0] == o.search_bytes(q), q
    finally:
        c.close()
        o.close()


def test_suffix_arrays_on_the_host_tier(tmp_path, search_env):
    rng = np.random.default_rng(12)
    data = comparison_text(rng)
    p = make_index(tmp_path, 'host', data)
    search_env(PSS_READER_HBM_BUDGET=0, PSS_SAMPLE_SHIFT=1)
    c = Case(p)
    try:
        assert c.r.residency['host_chunks'] == 1
        qs = comparison_queries(data)
        short = [q for q in qs if len(q) <= 256]
        light, _ = c.split(short)
        c.batch(light, R['SMALL_WAVE'] | R['KEY_SAMPLES'], single=0)
        c.singles(short, route_on=R['RESIDENT'], route_off=R['SMALL_BLOCK'])
        search_env(PSS_NO_SMALL_PATH=1, PSS_LANE_SEARCH_MIN=1)
        c.batch(qs, R['INTERVAL_LANE'] | R['MID'], single=0)
    finally:
        c.close()


# -------------------------------------------------------------------------------------------------- coverage guard --

def test_every_route_was_seen(request):
    """Runs last: the cases above FINISHED a batch on every route that include/pss.h names (overflowed routes do not
    count), so a threshold moved by a later change cannot silently drop a route from coverage.  It needs the whole
    module before it: with a subset of the module selected, or after a failure above, it has nothing to say."""
    hdr = pathlib.Path(ROOT, 'include', 'pss.h').read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r'#define PSS_ROUTE_(\w+)\s+0x([0-9a-fA-F]+)u', hdr)}
    assert defined == R
    here = [it for it in request.session.items if it.module is request.module]
    cases = {name for name in dir(request.module) if name.startswith('test_')} - {'test_every_route_was_seen'}
    if {it.originalname for it in here} != cases | {'test_every_route_was_seen'}:
        pytest.skip('only part of the module was selected')
    if request.session.testsfailed:
        pytest.skip('a case above failed')
    missing = [k for k, v in defined.items() if not SEEN[0] & v]
    assert not missing, missing
