"""What the GPU suites of the entry-level search kinds share: the index and reader set-ups, one check() of a batch against
its brute-force reference, the placement and fuzz-case scenarios, and the record of the routes that finished a batch.

A search kind (plain ids, anchored, all-terms, glob, case-insensitive, case-insensitive groups, near, edit) is a Kind:
its three Reader calls, its reference calls, its rule for `hits` and its route bits.  check(kind, ...) is the one
skeleton; each suite keeps a check() of its own signature that forwards to it.  tests/test_search_harness.py shows on a
fake reader, without a GPU, that check() rejects what it must for every kind."""
import ctypes
import dataclasses
import typing

import numpy as np

import pysubstringsearch
from pysubstringsearch_amd import _ffi, icase_variants
from tests.all_terms_ref import AllTermsRef
from tests.anchored_ref import AnchoredRef
from tests.edit_ref import EditRef
from tests.entry_id_ref import IdRef
from tests.glob_ref import GlobRef
from tests.icase_groups_ref import IcaseGroupsRef
from tests.icase_ref import IcaseRef
from tests.near_ref import NearRef

R = _ffi.ROUTES
FILLER = b'abcdefghijklmnop'    # marker queries use none of these bytes
INTERVAL = R['INTERVAL_LANE'] | R['INTERVAL_GROUP'] | R['INTERVAL_WAVE']
FUSED = R['SMALL_BLOCK'] | R['SMALL_WAVE']
NOT_GENERAL = R['MID'] | R['MID_OVERFLOW'] | FUSED | R['SMALL_OVERFLOW'] | R['RESIDENT'] | R['SA_ORDER']
SEEN = [0]                      # union of the routes that FINISHED a batch compared with a reference (and of the overflow bits):
                                # tests/test_search_edges_gpu.py adds its own and ends by asserting that every PSS_ROUTE_* bit is here


def finished(rt):
    """The route bits of a batch without the routes that overflowed (a later route answered in their place)."""
    if rt & R['SMALL_OVERFLOW']:
        rt &= ~FUSED
    if rt & R['MID_OVERFLOW']:
        rt &= ~R['MID']
    return rt


def filler(rng, n):
    return bytes(np.frombuffer(FILLER, np.uint8)[rng.integers(0, len(FILLER), n)])


def make_index(tmp_path, name, data, max_chunk_len=None):
    """HIP Writer over the lines of `data` (no '\\r' before a '\\n': the line rule would strip it)."""
    assert b'\r\n' not in data
    src = tmp_path / (name + '.txt')
    src.write_bytes(data)
    p = str(tmp_path / (name + '.idx'))
    w = pysubstringsearch.Writer(p, max_chunk_len)
    w.add_entries_from_file_lines(str(src))
    w.close()
    return p


def device_chunk(text):
    """(text, suffix array) of one chunk in HBM, as torch tensors."""
    import torch
    t = np.frombuffer(text, dtype=np.uint8).copy()
    sa = np.empty(len(text), dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(t.ctypes.data, sa.ctypes.data, len(text), 0))
    return torch.from_numpy(t).cuda(), torch.from_numpy(sa).cuda()


def device_reader(texts):
    """A reader filled through pss_reader_add_chunk_device: the only way to a text without a closing newline."""
    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = pysubstringsearch.Reader._from_handle(h)
    for t in texts:
        dt, ds = device_chunk(t)
        _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), len(t)))
    return r


def one_chunk(ref_cls, lines, closed=True):
    """(reader, reference, text) of one chunk handed over on the device."""
    data = b'\n'.join(lines) + (b'\n' if closed else b'')
    assert len(data) < 1_000_000
    return device_reader([data]), ref_cls([data]), data


def per_row(res):
    """The ids of an IdResult, one array per row of the batch."""
    out, pos = [], 0
    for c in res.counts.tolist():
        out.append(res.ids[pos:pos + c])
        pos += c
    return out


# ---- the kinds ------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Kind:
    """The places in which the check of one search kind differs from the others'.  `batch` is whatever the kind's calls
    take (a list, or a pair of a list and a per-batch argument); only the callables below look inside."""
    name: str
    ref_cls: type
    ids: typing.Callable            # (reader, batch) -> IdResult
    packed: typing.Callable         # (reader, batch) -> PackedResult
    counts: typing.Callable         # (reader, batch) -> list of counts
    rows: typing.Callable           # batch -> one tuple per query, as want / ordered take them after the reference
    want: typing.Callable           # (ref, *row) -> the row's ids, ascending
    ordered: typing.Optional[typing.Callable] = None        # (ref, *row) -> the row's ids in the stated order; None: none is stated
    want_hits: typing.Optional[typing.Callable] = None      # (ref, batch) -> `hits` exactly; None: hits >= the ids returned
    need: int = R['GENERAL']
    forbid: int = NOT_GENERAL | R['ANCHORED']
    plain: bool = False             # Reader.search_ids_batch: nothing is stated about hits, about the interval bit or about the
                                    # routes of search_batch_packed / count_multiple_bytes, and SA_ORDER follows result_order


def _listed(batch):
    return [(q,) for q in batch]


def _paired(batch):
    items, arg = batch
    return list(zip(items, [arg] * len(items) if isinstance(arg, (int, str)) else list(arg)))


def _near(name, ref_cls, want, **kw):
    return Kind(name, ref_cls,
                ids=lambda r, b: r.search_near_ids_batch(b[0], b[1], **kw),
                packed=lambda r, b: r.search_near_batch_packed(b[0], b[1], **kw),
                counts=lambda r, b: r.count_near_bytes(b[0], b[1], **kw),
                rows=_paired, want=want, ordered=lambda ref, p, k: ref.ordered_ids(p, k),
                want_hits=lambda ref, b: sum(ref.piece_hits(p, k) for p, k in _paired(b)))


def _icase_groups(name, what, ids, packed, counts, want):
    return Kind(name, IcaseGroupsRef,
                ids=lambda r, b: getattr(r, ids)(b, icase=True),
                packed=lambda r, b: getattr(r, packed)(b, icase=True),
                counts=lambda r, b: getattr(r, counts)(b, icase=True),
                rows=_listed, want=want, ordered=lambda ref, g: ref.ordered_ids(what, g),
                want_hits=lambda ref, b: ref.hits(what, b))


PLAIN = Kind('plain', IdRef,
             ids=lambda r, b: r.search_ids_batch(b),
             packed=lambda r, b: r.search_batch_packed(b),
             counts=lambda r, b: r.count_multiple_bytes(b),
             rows=_listed, want=lambda ref, q: ref.search_ids(q),
             forbid=R['MID'] | FUSED | R['RESIDENT'] | R['COUNTS'] | R['ANCHORED'], plain=True)
ANCHORED = Kind('anchored', AnchoredRef,
                ids=lambda r, b: r.search_anchored_ids_batch(b[0], b[1]),
                packed=lambda r, b: r.search_anchored_batch_packed(b[0], b[1]),
                counts=lambda r, b: r.count_anchored_bytes(b[0], b[1]),
                rows=_paired, want=lambda ref, q, anchor: ref.search_ids(q, anchor),
                need=R['GENERAL'] | R['ANCHORED'], forbid=NOT_GENERAL)
ALL_TERMS = Kind('all_terms', AllTermsRef,
                 ids=lambda r, b: r.search_all_ids_batch(b),
                 packed=lambda r, b: r.search_all_batch_packed(b),
                 counts=lambda r, b: r.count_all_bytes(b),
                 rows=_listed, want=lambda ref, g: ref.search_all_ids(g))
GLOB = Kind('glob', GlobRef,
            ids=lambda r, b: r.search_glob_ids_batch(b),
            packed=lambda r, b: r.search_glob_batch_packed(b),
            counts=lambda r, b: r.count_glob_bytes(b),
            rows=_listed, want=lambda ref, g: ref.search_glob_ids(g))
ICASE = Kind('icase', IcaseRef,
             ids=lambda r, b: r.search_icase_ids_batch(b),
             packed=lambda r, b: r.search_icase_batch_packed(b),
             counts=lambda r, b: r.count_icase_bytes(b),
             rows=_listed, want=lambda ref, g: ref.search_icase_ids(g),
             ordered=lambda ref, g: ref.ordered_ids(g, icase_variants(g)[0]))
ICASE_ALL = _icase_groups('icase_all', 'all', 'search_all_ids_batch', 'search_all_batch_packed', 'count_all_bytes',
                          lambda ref, g: ref.search_all_ids(g))
ICASE_GLOB = _icase_groups('icase_glob', 'glob', 'search_glob_ids_batch', 'search_glob_batch_packed', 'count_glob_bytes',
                           lambda ref, g: ref.search_glob_ids(g))
NEAR = _near('near', NearRef, lambda ref, p, k: ref.search_near_ids(p, k))
EDIT = _near('edit', EditRef, lambda ref, p, k: ref.search_edit_ids(p, k), edits=True)
KINDS = (PLAIN, ANCHORED, ALL_TERMS, GLOB, ICASE, ICASE_ALL, ICASE_GLOB, NEAR, EDIT)


# ---- the one check -----------------------------------------------------------------------------------------------------------

def check(kind, r, ref, batch, texts=True, order=True, interval=None):
    """batch through the three calls of kind on reader r against ref (the chunks r holds): the ids, then the counts, then
    the packed text, then entries_by_id_packed.  Returns the IdResult."""
    rows = kind.rows(batch)
    live = bool(rows) and r.num_chunks > 0
    routes = []

    def route_ok(st, counting):
        if not live:
            return
        route = st['route']
        routes.append(route)
        assert route & kind.need == kind.need, hex(route)
        assert not route & kind.forbid, hex(route)
        if kind.plain:
            assert bool(route & R['SA_ORDER']) == (r.result_order == 'sa'), hex(route)
            return
        assert bool(route & R['COUNTS']) == counting, hex(route)
        assert route & INTERVAL, hex(route)
        if interval is not None:
            assert route & INTERVAL == interval, hex(route)

    res = kind.ids(r, batch)
    st = r.last_stats()
    ids, counts = res.ids, res.counts.tolist()
    assert ids.dtype == np.uint64 and not ids.flags.writeable
    assert len(counts) == len(rows) and sum(counts) == ids.size
    assert st['entries'] == ids.size and st['result_bytes'] == 8 * ids.size and st['queries'] == len(rows)
    route_ok(st, False)
    hits = st['hits']
    if kind.want_hits is not None:
        want_hits = kind.want_hits(ref, batch) if live else 0
        assert hits == want_hits, ('hits', hits, want_hits)
    elif not kind.plain:
        assert hits >= ids.size
    assert counts == kind.counts(r, batch)
    if not kind.plain:
        st = r.last_stats()
        route_ok(st, True)
        assert st['hits'] == hits and st['entries'] == ids.size and st['queries'] == len(rows)
    pos = 0
    for row, c in zip(rows, counts):
        got = ids[pos:pos + c]
        pos += c
        want = kind.want(ref, *row)
        assert np.unique(got).size == got.size, (str(row)[:120], 'an id twice')
        assert np.array_equal(np.sort(got), want), (str(row)[:120], np.sort(got)[:8], want[:8])
        if order and kind.ordered is not None:
            assert np.array_equal(got, kind.ordered(ref, *row)), (str(row)[:120], 'order')
    # the same entries, in the same order, as the packed text result
    pk = kind.packed(r, batch)
    if not kind.plain:
        st = r.last_stats()
        route_ok(st, False)
        assert st['hits'] == hits and st['entries'] == ids.size and st['result_bytes'] == pk.data.size and st['queries'] == len(rows)
    by_id = r.entries_by_id_packed(ids)
    assert pk.counts.tolist() == counts
    assert np.array_equal(by_id.offsets, pk.offsets)
    assert np.array_equal(by_id.data, pk.data)
    assert by_id.counts.tolist() == [1] * ids.size
    if texts:       # ... and each is the text the reference has under that id
        want = [ref.entry(i) for i in ids.tolist()]
        data, o = pk.data.tobytes(), pk.offsets.tolist()
        assert [data[o[i]:o[i + 1]] for i in range(ids.size)] == want
        if kind.plain:
            assert r.entries_by_id(ids) == want
    if kind is ANCHORED:        # only the anchored calls set PSS_ROUTE_ANCHORED, and only here are they compared
        for rt in routes:
            SEEN[0] |= finished(rt)
    return res


# ---- recurring scenarios -----------------------------------------------------------------------------------------------------

def placement(kind, p, batch, search_env, order_multi=True, ref=None):
    """batch on index p (five chunks or more) however the reader is placed: whole, order='sa', two parts on one device, one
    shard of two, one suffix array on the host tier.  Every reader goes through check(); the ids are the whole reader's, in
    the order each placement states.  order_multi=False where the kind's stated order does not hold over several parts.
    Returns the whole reader's IdResult."""
    Reader = pysubstringsearch.Reader
    ref = kind.ref_cls.from_index(p) if ref is None else ref
    whole = Reader(p)
    try:
        # the line tables are absent until the id variant is called
        fresh = whole.residency
        text = kind.packed(whole, batch)
        counts = kind.counts(whole, batch)
        assert whole.residency == fresh
        base = check(kind, whole, ref, batch)
        assert whole.residency['hbm_bytes'] > fresh['hbm_bytes']
        assert base.counts.tolist() == counts == text.counts.tolist()
        again = kind.packed(whole, batch)
        assert np.array_equal(again.data, text.data) and np.array_equal(again.offsets, text.offsets)
        hbm = fresh['hbm_bytes']
        chunk_of = (base.ids >> np.uint64(32)).astype(np.int64)
        row_of = np.repeat(np.arange(base.counts.size), base.counts.astype(np.int64))
        assert (np.diff(chunk_of)[np.diff(row_of) == 0] >= 0).all()                       # chunk-major inside a row
        # order='sa' gives the identical result
        sa = Reader(p, order='sa')
        try:
            got = check(kind, sa, ref, batch)
            assert np.array_equal(got.ids, base.ids)
            pk = kind.packed(sa, batch)
            assert np.array_equal(pk.data, text.data) and np.array_equal(pk.offsets, text.offsets)
        finally:
            sa.close()
        # devices=[0, 0]: the merge is keyed by rows -- part-major inside a row; the ids of one file mean the same in every part
        multi = Reader(p, devices=[0, 0])
        try:
            got = check(kind, multi, ref, batch, order=order_multi)
            assert got.counts.tolist() == base.counts.tolist()
            key = np.lexsort((np.arange(base.ids.size), chunk_of % 2, row_of))
            assert np.array_equal(got.ids, base.ids[key])
        finally:
            multi.close()
        # shard (1, 2): the whole reader's ids of the odd chunks -- the file's chunk indexes -- in the same order
        shard = Reader(p, shard=(1, 2))
        try:
            sref = kind.ref_cls.from_index(p, keep=lambda c: c % 2 == 1)
            got = check(kind, shard, sref, batch)
            assert np.array_equal(got.ids, base.ids[chunk_of % 2 == 1])
            assert got.ids.size and ((got.ids >> np.uint64(32)) % np.uint64(2) == 1).all()
        finally:
            shard.close()
    finally:
        whole.close()
    # one suffix array too many for the budget: it stays in pinned host memory
    search_env(PSS_READER_HBM_BUDGET=hbm - 1, PSS_READER_AUTO_RESIDENCY=0)
    try:
        tier = Reader(p)
        try:
            assert tier.residency['host_chunks'] >= 1
            got = check(kind, tier, ref, batch)
            assert np.array_equal(got.ids, base.ids)
            assert tier.residency['host_chunks'] >= 1
        finally:
            tier.close()
    finally:
        search_env(PSS_READER_HBM_BUDGET=None, PSS_READER_AUTO_RESIDENCY=None)
    return base


def open_case(case, tmp_path, set_env, ref_classes, name):
    """(reader, [reference per class of ref_classes]) of a fuzz case, its switches set and the reader opened as drawn: the
    chunks handed over on the device, or the file as the Writer cut it -- whole, devices=[0, 0, 0], one shard, order='sa', or
    with one suffix array on the host tier."""
    Reader = pysubstringsearch.Reader
    set_env(**getattr(case, 'switches', {}))
    if case.setup == 'device':
        return device_reader(case.chunks), [cls(case.chunks) for cls in ref_classes]
    assert case.closed
    p = make_index(tmp_path, '%s%d' % (name, case.seed), b''.join(case.chunks), case.max_chunk_len)
    keep = (lambda c: True) if case.shard is None else (lambda c: c % case.shard[1] == case.shard[0])
    refs = [cls.from_index(p, keep=keep) for cls in ref_classes]
    held = [c for c in range(len(case.chunks)) if keep(c)]
    for ref in refs:                    # the Writer cut the file where the generator said it would
        assert [ch.index for ch in ref.chunks] == held and [ch.text for ch in ref.chunks] == [case.chunks[c] for c in held]
    if case.setup == 'devices':
        return Reader(p, devices=[0, 0, 0]), refs
    if case.setup == 'shard':
        return Reader(p, shard=case.shard), refs
    if case.setup == 'sa':
        return Reader(p, order='sa'), refs
    if case.setup == 'host':            # one suffix array too many for the budget: it stays in pinned host memory
        probe = Reader(p)
        hbm = probe.residency['hbm_bytes']
        probe.close()
        set_env(PSS_READER_HBM_BUDGET=hbm - 1, PSS_READER_AUTO_RESIDENCY=0)
        r = Reader(p)
        assert r.residency['host_chunks'] >= 1
        return r, refs
    return Reader(p), refs


# the six batches of a case of tests/search_fuzz_cases.py: (name, kind, the batch of the case)
FUZZ_BATCHES = (
    ('ids', PLAIN, lambda case: case.ids),
    ('anchored', ANCHORED, lambda case: ([p for p, _ in case.anchored], [k for _, k in case.anchored])),
    ('anchored_word', ANCHORED, lambda case: tuple(case.anchored_word)),
    ('all_terms', ALL_TERMS, lambda case: case.all_terms),
    ('glob', GLOB, lambda case: [g for _, _, g in case.glob]),
    ('icase', ICASE, lambda case: case.icase),
)


def run_case(case, tmp_path, set_env):
    """A case of tests/search_fuzz_cases.py: its six batches through check(), then one of them once more, which must
    return the identical ids -- no kind leaves state behind for another.  Returns {batch name: IdResult}."""
    r, refs = open_case(case, tmp_path, set_env, [kind.ref_cls for _, kind, _ in FUZZ_BATCHES], 'fuzz')
    interval = None if case.interval is None else R[case.interval]

    def run(i):
        _, kind, batch_of = FUZZ_BATCHES[i]
        return check(kind, r, refs[i], batch_of(case), order=case.setup != 'devices', interval=interval)

    try:
        got = [run(i) for i in range(len(FUZZ_BATCHES))]
        again = case.seed % len(FUZZ_BATCHES)
        res = run(again)
        assert np.array_equal(res.ids, got[again].ids) and np.array_equal(res.counts, got[again].counts), FUZZ_BATCHES[again][0]
        return {name: res for (name, _, _), res in zip(FUZZ_BATCHES, got)}
    finally:
        r.close()


# ---- rows and term bytes around a multiple of 64 -----------------------------------------------------------------------------
# The host driver rounds every region of a group batch's workspace to 64 bytes (csrc/search_layout.h): group offsets, flags
# and anchor bytes per row or term, the terms' bytes with 32 zero bytes behind them.  63, 64 and 65 rows whose term bytes
# add up to 31, 32 and 33 modulo 64 put every one of those regions on, just under and just over its rounding.

EDGE_ROWS = (63, 64, 65)
EDGE_BYTES = (31, 32, 33)


def edge_chunks():
    """A few hundred short entries of the filler alphabet in both cases (and five long ones), as one chunk and as three."""
    rng = np.random.default_rng(6464)
    lines = [filler(rng, int(rng.integers(0, 21))) for _ in range(300)] + [filler(rng, 80) for _ in range(5)]
    lines = [bytes(c - 32 if rng.random() < 0.25 else c for c in line) for line in lines]
    order = rng.permutation(len(lines))
    lines = [lines[int(i)] for i in order]
    cut = [b'\n'.join(lines[a:b]) + b'\n' for a, b in ((0, 100), (100, 200), (200, len(lines)))]
    return lines, ([b''.join(cut)], cut)


def edge_groups(rng, lines, rows, total_mod):
    """`rows` triples (a, b, ab): a and b cut from one entry left to right -- its start and its last byte, so the entry holds
    both, in order, apart -- and ab, the entry's start as long as both together.  The lengths of all a and b add up to total_mod
    modulo 64."""
    long_lines = [line for line in lines if len(line) >= 80]
    groups, total = [], 0
    while len(groups) < rows:
        last = len(groups) == rows - 1
        line = long_lines[int(rng.integers(0, len(long_lines)))] if last or rng.random() < 0.1 else lines[int(rng.integers(0, len(lines)))]
        if len(line) < 6:
            continue
        first = 2 + int(rng.integers(0, 2))
        if last:        # (the length that brings the total home: 2 .. 65 bytes)
            first = (total_mod - total - 1 - 2) % 64 + 2
        a, b = line[:first], line[-1:]
        assert len(line) > first + 1
        groups.append((a, b, line[:first + 1]))
        total += len(a) + len(b)
    assert total % 64 == total_mod and len(groups) == rows and all(len(a) + len(b) == len(ab) for a, b, ab in groups)
    return groups


def layout_edges(kind, batch_of, min_ids=1):
    """EDGE_ROWS x EDGE_BYTES batches of `kind` (batch_of: the triples of edge_groups as the kind's batch) through check() on the
    one-chunk and on the three-chunk reader: ids, counts and packed text against the brute-force reference."""
    lines, placements = edge_chunks()
    rng = np.random.default_rng(31 + 32 + 33)
    batches = [batch_of(edge_groups(rng, lines, rows, mod)) for rows in EDGE_ROWS for mod in EDGE_BYTES]
    for chunks in placements:
        r, ref = device_reader(chunks), kind.ref_cls(chunks)
        try:
            for batch in batches:
                assert len(kind.rows(batch)) in EDGE_ROWS
                assert check(kind, r, ref, batch).ids.size >= min_ids
        finally:
            r.close()


def edge_globs(groups, gap=b'*'):
    """The triples of edge_groups as glob patterns of two segments, every other one anchored at both ends."""
    return [(a + gap + b) if i % 2 else (b'*' + a + gap + b + b'*') for i, (a, b, _) in enumerate(groups)]
