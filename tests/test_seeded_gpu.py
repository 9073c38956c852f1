"""What only the one seeded verify path (seed_impl.h) can break: the case-insensitive and the near
batches share one host stage, one workspace layout and one kernel frame.  Every batch here goes through the check() of
tests/search_harness.py under its own kind -- near, case-insensitive, case-insensitive groups and globs, plain ids: ids,
packed text and counts against the brute-force references, in full.
  1. The kinds alternate on one reader: void flags, budgets, the overflow flag and the seed positions of an earlier batch
     of the other kind and another size lie in the same grow-only workspace slot.
  2. Seed positions are per QUERY: neighbours in one batch differ in both seed position and spelling count, and every
     pattern has decoys laid out around a neighbour's position."""
import numpy as np
import pytest

from pysubstringsearch_amd import glob_parse, icase_variants
from tests.entry_id_ref import IdRef
from tests.icase_groups_ref import IcaseGroupsRef
from tests.icase_ref import IcaseRef
from tests.near_ref import NearRef
from tests.search_harness import ICASE, ICASE_ALL, ICASE_GLOB, NEAR, PLAIN, check, device_reader, per_row

pytestmark = pytest.mark.gpu


def test_kinds_alternate_on_one_reader():
    chunks = [[b'Error: TIMEOUT after 500 ms', b'get /Admin 500', b'retry on error, timeout', b'tineout n 500', b'abcdefgh',
               b'GET /x/admin/y 500', b'', b'eRRoR TimeOut'],
              [b'timeouT', b'error', b'POST /admin 500', b'get /admin 5000', b'TIMEOUT ERROR RETRY', b'retry agaim', b'N 500',
               b'tiMeout error'],
              [b'Get /ADMIN 500', b'ERROR timeout retry', b'ximeoux', b'retsy afain', b'admin', b'an 500 timeoutimeout',
               b'error', b'get /adnin 500 eRROr TIMEOUT']]
    texts = [b'\n'.join(lines) + b'\n' for lines in chunks]
    texts[-1] = texts[-1][:-1]                      # the last entry of the last chunk is unterminated
    assert all(len(t) < 300 and len(lines) == 8 for t, lines in zip(texts, chunks))
    refs = {'near': NearRef(texts), 'icase': IcaseRef(texts), 'groups': IcaseGroupsRef(texts), 'plain': IdRef(texts)}
    near5, budgets5 = [b'timeout', b'tineout', b'err\nor!', b'retry again', b'admin'], [0, 1, 2, 3, 1]
    icase3 = [b'500', b'N 500', b'TIMEOUT']
    assert [len(icase_variants(p)[1]) for p in icase3] == [1, 2, 32]
    assert b'\n' in near5[2] and b'\n' not in icase3[2]        # the pattern at the void one's index is a live one
    groups = [([b'error', b'TIMEOUT'], [b'retry']), [b'ADMIN', b'get']]
    globs = [b'get */ADMIN* 500', b'error*']
    assert glob_parse(globs[0])[1] == 3                             # both anchors
    near2, budgets2 = [b'timeout', b'GET /admin'], [1, 2]
    r = device_reader(texts)
    try:
        for _ in range(2):
            res = per_row(check(NEAR, r, refs['near'], (near5, budgets5)))
            assert res[0].size and res[1].size > res[0].size and res[2].size == 0 and res[3].size and res[4].size
            res = per_row(check(ICASE, r, refs['icase'], icase3))
            assert all(x.size >= 3 for x in res)
            res = per_row(check(ICASE_ALL, r, refs['groups'], groups))
            assert all(x.size for x in res)
            res = per_row(check(ICASE_GLOB, r, refs['groups'], globs))
            assert all(x.size for x in res)
            res = per_row(check(NEAR, r, refs['near'], (near2, budgets2)))
            assert all(x.size for x in res)
            res = check(PLAIN, r, refs['plain'], [b'timeout', b'500', b'ERROR', b'nope'])
            assert all(c > 0 for c in res.counts.tolist()[:3]) and res.counts[3] == 0
    finally:
        r.close()


def seed_position_case():
    """(patterns, texts) of test_seed_positions_are_per_query, under PSS_ICASE_SEED_LETTERS=2."""
    # A: one letter, its own seed at 0, 2 spellings (under two seed letters a seed of ONE letter is the whole pattern: a longer
    # window would take the next letter in); B: the seed `c12d34` at 2, a proper sub-window, 4 spellings -- the most two letters
    # give; C: letterless, its own seed.  Neighbours differ in both position and spelling count.
    patterns = [b'1a234', b'abc12d34', b'#=+']
    chunk0 = [b'C12d34abC12d3',             # B's seed at the chunk's first byte: di < its position, rejected before anything is read
              b'..1A234..',                 # A, mangled
              b'..1a2x4 A234 1a23',         # A's decoy: near misses, 2 bytes into the entry as B's position would have it
              b'ABc12D34',                  # B, mangled, at the entry's start
              b'zzC12d34 abc12d3 bc12D34']  # B's decoys: the seed stands, with the wrong head before it, and the head without the seed
    chunk1 = [b'..#=+..',                   # C
              b'#= +#=',                    # C's decoy
              b'ab#=+c12d34',               # C again; B's seed 2 bytes behind C, B's head in front of it
              b'xAbC12d34 1A234']           # both again, unterminated
    return patterns, [b'\n'.join(chunk0) + b'\n', b'\n'.join(chunk1)]


def test_seed_positions_are_per_query(search_env):
    """A decoy cannot hold the whole pattern at a neighbour's position without holding it outright, so what a wrong position
    shows in is the real entries (the term is verified at the wrong start and missed) and the stated order; the decoys pin
    that seed hits outnumber matches, so the verify step decides."""
    search_env(PSS_ICASE_SEED_LETTERS=2)
    patterns, texts = seed_position_case()
    seeds = [icase_variants(p) for p in patterns]
    assert [(off, len(var)) for off, var in seeds] == [(0, 2), (2, 4), (0, 1)]
    assert seeds[1][1][0].lower() == b'c12d34' and len(icase_variants(b'ab12cd')[1]) == 4      # (4: the most the setting allows)
    ref, gref = IcaseRef(texts), IcaseGroupsRef(texts)
    assert [ref.search_icase_ids(p).size for p in patterns] == [2, 2, 2]
    assert ref.seed_hits(seeds[1][1][0]) == 6 and ref.seed_hits(b'1a2') == 4 and ref.seed_hits(b'#=') == 4
    r = device_reader(texts)
    try:
        res = per_row(check(ICASE, r, ref, patterns))
        assert [x.size for x in res] == [2, 2, 2]
        res2 = per_row(check(ICASE_ALL, r, gref, [[p] for p in patterns]))
        assert all(np.array_equal(a, b) for a, b in zip(res, res2))
    finally:
        r.close()
