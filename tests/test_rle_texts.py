"""tests/rle_texts.py on the CPU: every generator for every parameter tests/test_rle_edges_gpu.py uses (the construction
checks run inside the generators), the sizes the texts keep to, and the model's own algorithm -- run table, classes, ids,
generation order from the run heads' ranks, a stable sort by id -- held to the oracle's suffix array on exactly the planted
edges, before any kernel sees them.  Two cases are worked by hand, every model field written out."""
import numpy as np
import pytest

from tests import rle_texts as R
from tests import sa_edge_texts as E

MOST = 1 << 17          # most texts
LIMIT = 1 << 20         # every text but extent_far_case (and the two of test_four_passes, which are not generated here)


def _check(oracle, t, limit=MOST):
    assert t.dtype == np.uint8 and 2 <= t.size <= limit
    sa = oracle.sa(t)
    assert np.array_equal(R.model_sa(t, R.head_ranks(t, sa)), sa)
    return sa


@pytest.mark.parametrize('d', R.STRIP_DS)
def test_strip_cases(oracle, d):
    for rem in R.STRIP_REMS:
        t = R.strip_case(d, rem)
        _check(oracle, t)
        assert R.model(t).columns and not R.model(t, sort_knob=True).columns


def test_idbits_cases(oracle):
    for num_ids in R.IDBITS_NS:
        t = R.idbits_case(num_ids)
        _check(oracle, t)
        m = R.model(t)
        assert (m.id_bits, m.passes) == {2: (1, 1), 256: (8, 1), 257: (9, 2), 65536: (16, 2), 65537: (17, 3)}[num_ids]
        assert not m.columns and m.small == (num_ids <= 257)
    for num_ids in R.IDBITS_BIG_NS:
        t = R.idbits_case(num_ids, big=True)
        _check(oracle, t)
        m = R.model(t)
        assert (m.id_bits, m.passes, m.small) == {2: (1, 1, False), 256: (8, 1, False), 257: (9, 2, False)}[num_ids]
    # (four passes: what tests/test_rle_edges_gpu.py::test_four_passes relies on, at a size the CPU is quick with)
    for t in (R.from_runs([98, 97], [300, 1]), R.from_runs([97, 98], [300, 1])):
        sa = _check(oracle, t)
        assert np.array_equal(sa, np.arange(300, -1, -1) if t[0] == 98 else np.arange(301))
        assert R.model(t).num_ids == 301
    assert (1 << 24) < (1 << 24) + 2 <= (1 << 25)               # id_bits 25 for num_ids = 2^24 + 2


@pytest.mark.parametrize('clause', R.COLUMNS_CLAUSES)
def test_columns_cases(oracle, clause):
    holds, fails = R.columns_case(clause, 'holds'), R.columns_case(clause, 'fails')
    _check(oracle, holds)
    _check(oracle, fails)
    assert R.model(holds).columns and not R.model(fails).columns
    assert not R.model(holds, sort_knob=True).columns


@pytest.mark.parametrize('S', R.BLOCK_SS)
def test_block_cases(oracle, S):
    _check(oracle, R.block_case(S))


@pytest.mark.parametrize('d', R.CHUNK_DS)
def test_chunk_cases(oracle, d):
    _check(oracle, R.chunk_case(d))


@pytest.mark.parametrize('where', R.J0_WHERES)
def test_j0_cases(oracle, where):
    t = R.j0_case(where)
    sa = _check(oracle, t)
    assert np.array_equal(R.naive_head_ranks(t), R.head_ranks(t, sa))


@pytest.mark.parametrize('small', [False, True])
@pytest.mark.parametrize('r', R.TINY_RS)
def test_tiny_runs_cases(oracle, r, small):
    t = R.tiny_runs_case(r, small)
    sa = _check(oracle, t)
    assert np.array_equal(R.naive_head_ranks(t), R.head_ranks(t, sa))


@pytest.mark.parametrize('k', E.TIER_KS)
def test_tier_cases(oracle, k):
    _check(oracle, R.tier_case(k), LIMIT)


def test_closed_form_cases(oracle):
    for where in R.EXTENT_WHERES:
        for above in ((False, True) if where != 'none' else (False,)):
            t = R.extent_case(where, above)
            assert t.size <= MOST
            blocks, late = R.period_blocks(t, oracle.sa(t))          # (asserts the closed form's shape on libsais' order)
            pm = R.period_model(t)
            assert len(blocks) == pm.p and late.size == pm.n - pm.long_end
    # single: the outputs 16504 .. 16511 of one thread hold the last two slots of the block of rotation 3, ONE late slot
    # (16506) and the first slots of the block of rotation 1; the same at 27509
    t = R.fill_case(oracle.sa, 'single')
    assert t.size == 33010
    blocks, late = R.period_blocks(t, oracle.sa(t))
    assert blocks == [(3, 5499, 5), (5504, 5500, 0), (11007, 5499, 3), (16507, 5500, 1), (22010, 5499, 4), (27510, 5500, 2)]
    assert late.tolist() == [0, 1, 2, 5502, 5503, 11004, 11005, 11006, 16506, 22007, 22008, 22009, 27509]
    assert R.fill_group(blocks, late, t.size, 'single') == 16504 and R.fill_group(blocks, late, t.size, 'stretch') is None
    assert 16504 % 8 == 0 and 16504 < 11007 + 5499 - 1 and 11007 + 5499 == 16506 and 16507 < 16511
    # stretch: the outputs 32000 .. 32007 hold the last two slots of rotation 2, four late slots and the first of rotation 1
    t = R.fill_case(oracle.sa, 'stretch')
    assert t.size == 40007
    blocks, late = R.period_blocks(t, oracle.sa(t))
    assert blocks == [(0, 7997, 4), (8002, 7998, 0), (16004, 7997, 3), (24005, 7997, 2), (32006, 7998, 1)]
    assert late.tolist() == (list(range(7997, 8002)) + list(range(16000, 16004)) + list(range(24001, 24005)) + list(range(32002, 32006))
                             + [40004, 40005, 40006])
    assert R.fill_group(blocks, late, t.size, 'stretch') == 32000
    assert 32000 % 8 == 0 and 32000 < 24005 + 7997 - 1 and 24005 + 7997 == 32002 and 32006 < 32007
    t = R.extent_far_case(256)                                       # (the compute units of an MI355X)
    assert t.size == (8 << 20) + 5000
    blocks, late = R.period_blocks(t, oracle.sa(t))
    assert len(blocks) == 23 and late.size == 2 * 23 + 3 * 500 + 1


def test_closed_form_is_declined_or_taken_on_the_pinned_limits():
    """kPeriodMax, kPeriodTailMax and the screen's first n, as tests/test_sa_gpu.py pins them on the GPU."""
    w = np.random.default_rng(5).integers(97, 123, 1025).astype(np.uint8)
    assert R.period_model(np.resize(w[:1024], 1 << 17)).taken and not R.period_model(np.resize(w, 1 << 17)).taken
    ab = np.resize(np.array([97, 98], np.uint8), 32768)
    assert R.period_model(ab).taken and not R.period_model(ab[:32767]).taken and R.period_model(ab[:32767]).period == 0
    t = np.resize(np.array([97, 98, 99], np.uint8), 50000)
    for tail, taken in ((1024, True), (1025, False)):
        u = t.copy()
        u[50000 - tail] = 122
        pm = R.period_model(u)
        assert (pm.tail, pm.taken, pm.extent) == (tail, taken, 50000 - tail)
    assert R.period_of_head(np.full(8192, 97, np.uint8)) == 0          # one byte repeated is no word


def test_six_runs_by_hand(oracle):
    """aaa bb a cc aa b: every field of the model, worked by hand."""
    t = np.frombuffer(b'aaabbaccaab', dtype=np.uint8)
    m = R.model(t)
    a, b, c = 97, 98, 99
    assert (m.n, m.S) == (11, 6)
    assert m.start.tolist() == [0, 3, 5, 6, 8, 10] and m.L.tolist() == [3, 2, 1, 2, 2, 1]
    assert m.byte.tolist() == [a, b, a, c, a, b]
    assert m.type.tolist() == [1, 0, 1, 0, 1, 0]                       # next byte above: b > a, a < b, c > a, a < c, b > a, the end
    # classes (a, 1) = 195, (b, 0) = 196, (c, 0) = 198: longest runs 3, 2, 2; bases 0, 3, 5 (5 as well for the empty (b, 1)); 7 ids
    assert m.cls.tolist() == [195, 196, 195, 198, 195, 196]
    assert {q: int(m.cls_max[q]) for q in np.flatnonzero(m.cls_max)} == {195: 3, 196: 2, 198: 2}
    assert (int(m.cls_base[195]), int(m.cls_base[196]), int(m.cls_base[197]), int(m.cls_base[198])) == (0, 3, 5, 5)
    assert m.num_ids == 7 and m.id_bits == 3 and m.passes == 1        # 2, 4 < 7 <= 8
    # type 1: [top - L, top) with top = 0 + 3; type 0: [base, base + L)
    assert list(zip(m.lo.tolist(), m.hi.tolist())) == [(0, 3), (3, 5), (2, 3), (5, 7), (1, 3), (3, 4)]
    assert (m.NB, m.idpad, m.nchunks, m.nseg) == (1, 64, 1, 1)
    assert m.clauses == {'a': False, 'b': False, 'c': False, 'd': False, 'e': True}      # 11 < 4096, 24 > 11, 256 > 11, 256 > 88
    assert not m.columns and m.small
    # the run heads in order: aaab.. < aab$ < acc.. (type 1: the longer run first), then b$ < bba.., then cc
    ranks = [0, 4, 2, 5, 1, 3]
    assert R.naive_head_ranks(t).tolist() == ranks
    sar, j0, order = R.generation_order(m, ranks)
    assert sar.tolist() == [0, 4, 2, 5, 1, 3] and j0 == 0
    assert order.tolist() == [5, 3, 1, 4, 0, 2]                        # the last run, then the runs before 4, 2, 5, 1, 3
    # generated: 10 | 6 7 | 3 4 | 8 9 | 0 1 2 | 5 with ids 3 | 6 5 | 4 3 | 1 2 | 0 1 2 | 2; the stable sort by id:
    want = [0, 8, 1, 9, 2, 5, 10, 4, 3, 7, 6]
    assert R.model_sa(t, ranks).tolist() == want
    assert oracle.sa(t).tolist() == want


def test_twelve_periodic_bytes_by_hand(oracle):
    """abcabcabcabc: every field of the period model, worked by hand."""
    t = np.frombuffer(b'abcabcabcabc', dtype=np.uint8)
    pm = R.period_model(t)
    assert pm.p == 3                                                   # 2 fails at once (a != c); 3 holds and 4 * 3 <= 12
    assert (pm.first, pm.m, pm.tail, pm.margin) == (None, 12, 0, 7)
    assert pm.desc                                                     # the repetition runs into the end of the text
    assert not pm.screened and not pm.taken and (pm.period, pm.extent) == (0, 0)      # 12 < 32768: the screen does not look
    assert R.period_of_head(np.frombuffer(b'abcabcabcabd', dtype=np.uint8)) == 0      # c against d inside the head
    assert R.period_of_head(np.frombuffer(b'abcabcabcab', dtype=np.uint8)) == 0       # 4 * 3 > 11
    assert R.period_of_head(np.frombuffer(b'abababab', dtype=np.uint8)) == 2
    # the same word at the first size the screen looks at, 32769 = 3 * 10923 bytes: 3 blocks and 2 * 3 + 1 late suffixes
    # (from 32762 on), descending; rotation abc: late 32766, 32763, then 10921 long ones; bca: 32767, 32764, then 10921;
    # cab: 32768, 32765, 32762, then 10920
    big = np.resize(t[:3], 32769)
    pm = R.period_model(big)
    assert (pm.p, pm.first, pm.m, pm.tail, pm.margin, pm.long_end) == (3, None, 32769, 0, 7, 32762)
    assert pm.taken and pm.desc and (pm.period, pm.extent) == (3, 32769)
    blocks, late = R.period_blocks(big, oracle.sa(big))
    assert late.tolist() == [0, 1, 10923, 10924, 21846, 21847, 21848]
    assert blocks == [(2, 10921, 0), (10925, 10921, 1), (21849, 10920, 2)]
    # ... and with d for the last c: the first mismatch is t[32765] = c against t[32768] = d, one byte of tail, ascending
    big[32768] = 100
    pm = R.period_model(big)
    assert (pm.p, pm.first, pm.m, pm.tail, pm.margin, pm.long_end) == (3, 32765, 32768, 1, 9, 32759)
    assert pm.taken and not pm.desc and (pm.period, pm.extent) == (3, 32768)      # d > W[32768 % 3] = c
