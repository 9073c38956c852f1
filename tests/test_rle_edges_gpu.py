"""The run-length path and the closed form for periodic texts (rle_build.hip) on their limits: the 16-byte strips and
4096-byte tiles of the run table, the 512 classes and the id arithmetic on both sides of a radix pass, every clause that
chooses between the matrix walk and the stable sort, blocks / segments / chunks of the walk, the 8-slot threads of the
sort expansion, the group-size tiers of the rank rounds on the reduced string, and the extent and fill kernels of the
closed form.  The texts come from tests/rle_texts.py, which checks on the CPU that they hold what a case is about; the
statistics are compared with its numpy model, and every suffix array with the oracle's for equality -- it is unique, so
there is no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from tests import rle_texts as R
from tests import sa_edge_texts as E
from tests.util import sa_device

pytestmark = pytest.mark.gpu

_CACHE = {}


def _case(oracle, key, make):
    """(text, the oracle's suffix array): made once per session, never written to."""
    if key not in _CACHE:
        t = np.ascontiguousarray(make())
        want = oracle.sa(t)
        t.setflags(write=False)
        want.setflags(write=False)
        _CACHE[key] = (t, want)
    return _CACHE[key]


def _sa_at_offset(t, off, st):
    """pss_sa_build_device on a text that lies `off` bytes into a 16-byte aligned device buffer."""
    import torch
    from pysubstringsearch_amd import _ffi
    n = t.size
    big = torch.zeros(n + 64, dtype=torch.uint8, device='cuda')
    big[off:off + n] = torch.from_numpy(np.array(t)).cuda()
    assert big.data_ptr() % 16 == 0
    dSA = torch.empty(n, dtype=torch.int32, device='cuda')
    raw = _ffi.SaStats()
    _ffi.check(_ffi.lib.pss_sa_build_device(big.data_ptr() + off, dSA.data_ptr(), n, 0, 0, ctypes.byref(raw)))
    st.update(raw.as_dict())
    return dSA.cpu().numpy()


def _rle_build(monkeypatch, t, want, expansion, note, off=0):
    """One build through the run-length path, its statistics held to the model."""
    monkeypatch.setenv('PSS_RLE', '1')
    monkeypatch.setenv('PSS_PERIOD', '0')
    if expansion == 'sort':
        monkeypatch.setenv('PSS_RLE_SORT', '1')
    else:
        monkeypatch.delenv('PSS_RLE_SORT', raising=False)
    m = R.model(t, sort_knob=expansion == 'sort')
    st = {}
    sa = _sa_at_offset(t, off, st) if off else sa_device(np.array(t), st)
    assert np.array_equal(sa, want), note
    assert st['runs'] == m.S, (note, st['runs'], m.S)
    assert st['rle_id_bits'] == m.id_bits, (note, st['rle_id_bits'], m.id_bits)
    assert st['rle'] == (2 if m.columns else 1), (note, st['rle'], m.clauses)
    assert st['period_path'] == 0, note
    return st


EXPANSIONS = ('auto', 'sort')


# ---- run table -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('expansion', EXPANSIONS)
@pytest.mark.parametrize('d', R.STRIP_DS)
def test_run_starts_on_strip_word_and_tile_edges(oracle, monkeypatch, d, expansion):
    """R.strip_case: run starts at every residue mod 16 with neighbours that differ in bit 7, in bit 0 and in all bits, at
    RL_TILE * k + d, n % 16 in {0, 1, 15} -- and the same text at a device pointer 1 and 15 bytes off alignment, where
    rle_count / rle_starts and sa_symbols_kernel take their scalar branches everywhere.  `runs` is sa_symbols_kernel's
    count and the build compares it with the run table's, so S from the model pins both."""
    for rem in R.STRIP_REMS:
        t, want = _case(oracle, ('strip', d, rem), lambda: R.strip_case(d, rem))
        for off in (0, 1, 15):
            _rle_build(monkeypatch, t, want, expansion, (d, rem, off), off)


# ---- classes and ids -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num_ids', R.IDBITS_NS)
def test_number_of_ids_on_both_sides_of_a_radix_pass(oracle, monkeypatch, num_ids):
    """R.idbits_case: exactly 2, 256, 257, 65536, 65537 ids -- id_bits 1, 8, 9, 16, 17; classes of bytes 0 and 255, both id
    formulas, the last run of type 0.  `columns` is false for all five, so the expansion is the sort whatever PSS_RLE_SORT
    says: for 2, 256 and 257 ids (n <= 4096) the single-workgroup sort, where the number of passes plays no part; for 65536
    and 65537 ids the radix sort in two passes (final_buf 0) and three (final_buf 1)."""
    t, want = _case(oracle, ('idbits', num_ids), lambda: R.idbits_case(num_ids))
    m = R.model(t)
    assert not m.columns and m.small == (num_ids <= 257) and m.passes == {2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3}[num_ids]
    st = _rle_build(monkeypatch, t, want, 'auto', num_ids)
    assert st['rle'] == 1


@pytest.mark.parametrize('expansion', EXPANSIONS)
@pytest.mark.parametrize('num_ids', R.IDBITS_BIG_NS)
def test_passes_and_buffer_parity_of_the_sort_expansion(oracle, monkeypatch, num_ids, expansion):
    """R.idbits_case(big): 2, 256 and 257 ids in more than 4096 bytes, so the sort expansion is the radix sort proper: one
    pass for id_bits 1 and 8 (final_buf = 1: the last pass writes SA through buffer 1), two for id_bits 9 (final_buf = 0).
    With 65536 and 65537 ids above (two and three passes) and test_four_passes that is every number of passes and both
    parities on each side of a pass.  Without PSS_RLE_SORT the texts of 256 and 257 ids take the matrix walk instead."""
    t, want = _case(oracle, ('idbits big', num_ids), lambda: R.idbits_case(num_ids, big=True))
    m = R.model(t)
    assert not m.small and (m.id_bits, m.passes) == {2: (1, 1), 256: (8, 1), 257: (9, 2)}[num_ids]
    st = _rle_build(monkeypatch, t, want, expansion, (num_ids, expansion))
    assert st['rle'] == (2 if expansion == 'auto' and num_ids != 2 else 1)


@pytest.mark.parametrize('order', ['descending', 'ascending'])
def test_four_passes(order):
    """Four passes of the sort expansion need num_ids > 2^24, and a class's ids are its longest run: nothing shorter than
    one run of 2^24 + 1 bytes reaches that code.  b^(n-1) a has the suffix array n-1, n-2, ..., 0 and a^(n-1) b has 0, 1,
    ..., n-1 (n = 2^24 + 2), so they are compared with np.arange, not with libsais.  num_ids = n makes id_bits 25, and the
    expansion is the sort because clause (c), idpad * 4 <= n, fails on its own.  The path is the automatic choice here."""
    n = (1 << 24) + 2
    t = np.full(n, 98 if order == 'descending' else 97, np.uint8)
    t[-1] = 97 if order == 'descending' else 98
    m = R.model(t)
    assert m.num_ids == n and m.passes == 4 and [k for k, v in m.clauses.items() if not v] == ['c']
    st = {}
    sa = sa_device(t, st)
    assert np.array_equal(sa, np.arange(n - 1, -1, -1, dtype=np.int32) if order == 'descending' else np.arange(n, dtype=np.int32))
    assert (st['runs'], st['rle_id_bits'], st['rle'], st['period_path']) == (2, 25, 1, 0)


# ---- which expansion -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clause', R.COLUMNS_CLAUSES)
def test_each_clause_of_columns_from_both_sides(oracle, monkeypatch, clause):
    """R.columns_case: two texts one byte apart, the clause met with equality in one and missed in the other, every other
    clause true in both -- the walk on one side, the sort on the other, the oracle's bytes on both; and the sort on both
    with PSS_RLE_SORT."""
    rle = {}
    for side in ('holds', 'fails'):
        t, want = _case(oracle, ('columns', clause, side), lambda: R.columns_case(clause, side))
        rle[side] = _rle_build(monkeypatch, t, want, 'auto', (clause, side))['rle']
        _rle_build(monkeypatch, t, want, 'sort', (clause, side, 'sort'))
    assert rle == {'holds': 2, 'fails': 1}


# ---- matrix walk -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('expansion', EXPANSIONS)
@pytest.mark.parametrize('S', R.BLOCK_SS)
def test_blocks_and_scan_segments(oracle, monkeypatch, S, expansion):
    """R.block_case: 63, 64, 65 runs (idle lanes in the last block of 64), 4096, 4097, 8193 runs (one, two and three segments
    of the column scan), and 1 and 2 runs, which can only take the sort."""
    t, want = _case(oracle, ('block', S), lambda: R.block_case(S))
    st = _rle_build(monkeypatch, t, want, expansion, S)
    assert st['rle'] == (2 if S > 2 and expansion == 'auto' else 1)


@pytest.mark.parametrize('expansion', EXPANSIONS)
@pytest.mark.parametrize('d', R.CHUNK_DS)
def test_full_chunk_shortcut_with_equality(oracle, monkeypatch, d, expansion):
    """R.chunk_case: run lengths 64 k + d.  d = 0: every chunk of 64 ids takes the `full` shortcut, at the ends of a run with
    equality in mylo <= id0 and myhi >= id0 + 64; d = +-1: the same chunks go through the per-id loop."""
    t, want = _case(oracle, ('chunk', d), lambda: R.chunk_case(d))
    _rle_build(monkeypatch, t, want, expansion, d)


@pytest.mark.parametrize('expansion', EXPANSIONS)
@pytest.mark.parametrize('where', R.J0_WHERES)
def test_slot_of_the_first_run(oracle, monkeypatch, where, expansion):
    """R.j0_case: rle_ord skips j0 = 0, j0 = S - 1 and a j0 in the middle."""
    t, want = _case(oracle, ('j0', where), lambda: R.j0_case(where))
    _rle_build(monkeypatch, t, want, expansion, where)


# ---- expansion by sort -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('small', [False, True])
@pytest.mark.parametrize('r', R.TINY_RS)
def test_expand_threads_across_tiny_runs(oracle, monkeypatch, r, small):
    """R.tiny_runs_case: runs of 1 and 2 bytes, 4 to 8 of them under one thread's 8 slots, n % 8 = 0, 1, 7 (vector and
    scalar stores), above one radix tile and -- small -- within it (the single-workgroup sort, `small = n <= 4096`)."""
    t, want = _case(oracle, ('tiny', r, small), lambda: R.tiny_runs_case(r, small))
    for expansion in EXPANSIONS:
        st = _rle_build(monkeypatch, t, want, expansion, (r, small, expansion))
        assert st['rle'] == 1


# ---- reduced string --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', E.TIER_KS)
def test_tiers_of_the_rank_rounds_on_the_reduced_string(oracle, monkeypatch, k):
    """R.tier_case: groups of exactly k tied run heads that outlive two rank rounds of suffix_rounds_integer (Rounds
    without codes, h0 = 1), k on both sides of GS_CAP = 512, MID_CAP = 4096 and two tiles of 4096.  As in the text path
    (tests/test_sa_edges_gpu.py), big_elems counts the members that stayed with the chained sorts or the segmented merge: the
    largest group is exactly k and the build hands its statistics to the rounds, so it is zero up to MID_CAP and positive
    beyond -- which also shows that the group reached the rounds whole."""
    t, want = _case(oracle, ('tier', k), lambda: R.tier_case(k))
    for expansion in EXPANSIONS:
        st = _rle_build(monkeypatch, t, want, expansion, (k, expansion))
        print(k, expansion, 'big_elems', st['big_elems'], 'rounds', st['rounds'])
        assert (st['big_elems'] > 0) == (k > E.MID_CAP), (k, expansion, st['big_elems'])


# ---- closed form -----------------------------------------------------------------------------------------------------

def _period_build(t, want, note):
    pm = R.period_model(t)
    st = {}
    sa = sa_device(np.array(t), st)
    assert (st['period'], st['period_extent'], st['period_path']) == (pm.period, pm.extent, 1 if pm.taken else 0), note
    assert st['rle'] == 0, note
    assert np.array_equal(sa, want), note
    return pm


@pytest.mark.parametrize('where,above', [(w, a) for w in R.EXTENT_WHERES for a in (False, True) if w != 'none' or not a])
def test_extent_of_the_repetition(oracle, where, above):
    """R.extent_case: the first mismatch at the last position of a thread's 16, at the first of the next thread's, at the last
    position compared, and absent; the break byte below and above the word's letter (descending and ascending blocks).
    period, period_extent and period_path are the model's."""
    t, want = _case(oracle, ('extent', where, above), lambda: R.extent_case(where, above))
    pm = _period_build(t, want, (where, above))
    assert pm.taken and pm.desc == (not above or where == 'none')


def test_extent_found_in_the_second_grid_stride(oracle):
    """R.extent_far_case: one grid stride of period_extent_kernel is CUs * 8 * 256 * 16 bytes (8 MiB on 256 compute units),
    so only a text longer than that sends a thread round its loop a second time; the break byte lies 500 bytes before the
    end, where only second-stride threads compare."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t, want = _case(oracle, ('far', cus), lambda: R.extent_far_case(cus))
    pm = _period_build(t, want, cus)
    assert pm.taken and pm.extent == t.size - 500


@pytest.mark.parametrize('kind', R.FILL_KINDS)
def test_fill_across_block_boundaries_and_late_slots(oracle, kind):
    """R.fill_case: a group of 8 outputs of period_fill_kernel that holds, strictly inside, the end of a rotation block, late
    slots -- a single one, or a stretch of four -- and the start of the next block."""
    t, want = _case(oracle, ('fill', kind), lambda: R.fill_case(oracle.sa, kind))
    pm = _period_build(t, want, kind)
    assert pm.taken
