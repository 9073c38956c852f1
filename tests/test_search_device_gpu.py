"""The device-resident result (Reader.search_batch_device, SEARCH_DEVICE) on every pipeline that can produce it: the mid
pipeline, the general pipeline (by switch, by overflow of the mid pipeline, in suffix-array order), the zero-hit tail,
the empty batch and a reader without chunks.  Every batch is compared with search_batch_packed on the same reader and
with the brute-force reference (tests/search_ref.py), and last_stats()['route'] proves the pipeline that answered.
One index of three chunks of about 20 KB, filler and marker lines in the style of tests/test_search_edges_gpu.py; one
entry holds its marker twice, so the per-entry dedupe matters."""
import ctypes

import numpy as np
import pytest

import pysubstringsearch
from pysubstringsearch_amd import _ffi
from tests.search_harness import filler
from tests.search_ref import SearchRef

pytestmark = pytest.mark.gpu

R = _ffi.ROUTES
MID_CAP = 65536                 # hits the mid pipeline takes (search.hip, MID_MAX)
MISSES = [b'\x01MISS0', b'QQ', b'MKAx~', b'zzzzzzzzzzzzzzzzzzzz']
MIXED = [b'MKA', b'\x01MISS0', b'MKB', b'MKD', b'abc', b'QQ', b'MKD' + b'x', b'MKA\n']      # hits and misses, 8 queries


class Index:
    """The index, its reference and a memo of the reference's answers: built once, read by every test."""

    def __init__(self, tmp):
        rng = np.random.default_rng(11)
        lines = [filler(rng, int(rng.integers(20, 60))) for _ in range(1500)]
        for k, m in ((40, b'MKA'), (7, b'MKB')):
            for i in rng.integers(0, len(lines), k):
                lines[i] = lines[i][:9] + m + lines[i][9:]
        lines[700] = b'MKDx' + filler(rng, 12) + b'MKDx' + filler(rng, 5)        # its marker twice: one entry, two hits
        data = b'\n'.join(lines) + b'\n'
        src = tmp / 'dev.txt'
        src.write_bytes(data)
        self.path = str(tmp / 'dev.idx')
        w = pysubstringsearch.Writer(self.path, len(data) // 3 + 200)
        w.add_entries_from_file_lines(str(src))
        w.close()
        self.ref = SearchRef.from_index(self.path)
        assert len(self.ref.chunks) == 3 and all(15000 < len(c.text) < 30000 for c in self.ref.chunks)
        self.memo = {}

    def want(self, q):
        if q not in self.memo:
            self.memo[q] = sorted(self.ref.search(q))
        return self.memo[q]


@pytest.fixture(scope='module')
def index(tmp_path_factory):
    return Index(tmp_path_factory.mktemp('search_device'))


@pytest.fixture
def reader(index):
    r = pysubstringsearch.Reader(index.path)
    yield r
    r.close()


def cut(data, starts, num_bytes):
    """The entries of a packed result given as entry starts and the closing num_bytes."""
    edges = list(starts) + [num_bytes]
    return [data[edges[i]:edges[i + 1]] for i in range(len(edges) - 1)]


def check(r, qs, want, route=0, no_route=0):
    """search_batch_device(qs) on r against search_batch_packed(qs) and the reference answers `want` (one sorted list
    per query).  Returns the device batch's route."""
    dr = r.search_batch_device(qs)
    rt = r.last_stats()['route']
    pk = r.search_batch_packed(qs)
    counts = dr.counts.cpu().numpy().astype(np.uint64)
    assert counts.tolist() == pk.counts.tolist() == [len(w) for w in want]
    starts = dr.starts.cpu().numpy().tolist()
    data = dr.data.cpu().numpy().tobytes()
    # num_entries, num_bytes and the arrays agree with each other and with the packed result
    assert len(starts) == int(counts.sum()) == len(pk.offsets) - 1
    assert dr.num_bytes == len(data) == int(pk.offsets[-1])
    assert starts == sorted(starts) and (not starts or (starts[0] == 0 and starts[-1] <= dr.num_bytes))
    got = cut(data, starts, dr.num_bytes)
    packed = cut(pk.data.tobytes(), pk.offsets.tolist()[:-1], int(pk.offsets[-1]))
    pos = 0
    for q, w in zip(qs, want):
        assert sorted(got[pos:pos + len(w)]) == sorted(packed[pos:pos + len(w)]) == w, q[:20]
        pos += len(w)
    assert rt & route == route and not rt & no_route, (hex(rt), hex(route), hex(no_route))
    return rt


def test_mid_pipeline(index, reader):
    want = [index.want(q) for q in MIXED]
    assert len(index.want(b'MKD')) == 1 and sum(index.ref.hits(b'MKD')) == 2         # the entry that holds its marker twice
    assert [bool(w) for w in want] == [True, False, True, True, True, False, True, False]
    check(reader, MIXED, want, R['MID'], R['MID_OVERFLOW'] | R['GENERAL'])


def test_general_pipeline(index, reader, search_env):
    search_env(PSS_NO_MID_PIPELINE=1)
    check(reader, MIXED, [index.want(q) for q in MIXED], R['GENERAL'], R['MID'])


def test_mid_overflow_into_general(index, reader):
    per_query = sum(index.ref.hits(b'a'))
    nq = MID_CAP // per_query + 1
    assert nq * per_query > MID_CAP and nq * 3 <= MID_CAP           # more hits than the cap, on pairs the mid pipeline takes
    check(reader, [b'a'] * nq, [index.want(b'a')] * nq, R['MID'] | R['MID_OVERFLOW'] | R['GENERAL'])


def test_only_misses(index, reader, search_env):
    for env in ({}, {'PSS_NO_MID_PIPELINE': 1}):                   # the mid pipeline with nothing to emit; the zero-hit tail
        search_env(**env)
        assert not any(index.want(q) for q in MISSES)
        rt = check(reader, MISSES, [[] for _ in MISSES], R['GENERAL'] if env else R['MID'])
        assert not rt & R['MID_OVERFLOW']
        dr = reader.search_batch_device(MISSES)
        assert dr.counts.cpu().tolist() == [0] * len(MISSES) and dr.starts.numel() == 0 and dr.data.numel() == 0 and dr.num_bytes == 0


def test_no_query(reader):
    check(reader, [], [])
    dr = reader.search_batch_device([])
    assert dr.counts.numel() == 0 and dr.starts.numel() == 0 and dr.data.numel() == 0 and dr.num_bytes == 0


def test_reader_without_chunks():
    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = pysubstringsearch.Reader._from_handle(h)
    try:
        assert r.num_chunks == 0
        qs = [b'MKA', b'a', b'']
        check(r, qs, [[], [], []])
        dr = r.search_batch_device(qs)
        assert dr.counts.cpu().tolist() == [0, 0, 0] and dr.starts.numel() == 0 and dr.data.numel() == 0 and dr.num_bytes == 0
    finally:
        r.close()


def test_suffix_array_order(index):
    r = pysubstringsearch.Reader(index.path, order='sa')
    try:
        check(r, MIXED, [index.want(q) for q in MIXED], R['SA_ORDER'] | R['GENERAL'], R['MID'])
    finally:
        r.close()
