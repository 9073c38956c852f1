"""The shared check() of tests/search_harness.py on a fake reader, without a GPU: for each of the nine search kinds an
honest reader (every answer taken straight from the kind's brute-force reference) passes, and each single corruption of
its answers -- an id, a count, the packed text, a statistic, a route bit -- makes check() raise, as the kind's own check()
did before the nine became one."""
import types

import numpy as np
import pytest

from pysubstringsearch_amd import IdResult, PackedResult
from tests import search_harness as H

R = H.R
EMPTY = np.zeros(0, dtype=np.uint64)
CHUNKS = [b'ab\nAb a\n\nabab\nbaB\naabb\nb\nabAB ab\nzab\naB\nbbaa\nabba\n',
          b'Abab\nba\nab ab\na\nBA ab\n\nbbab\naabb ab\nAB\nabab\n',
          b'ab\nbaba\naAbB\nab a\nbab\nABAB\nabab ab']                    # (the last entry is unterminated)
BATCHES = {
    'plain': [b'a', b'ab', b'zz', b'', b'a\nb', b'Ab'],
    'anchored': ([b'a', b'ab', b'zz', b'', b'a\nb', b'B'], ['start', 'end', 'entry', 'start', 'end', 'entry']),
    'all_terms': [[b'a', b'b'], ([b'a'], [b' ']), [b'zz'], [b'ab', b'ba'], [b'a\nb', b'a'], [b'A', b'B']],
    'glob': [b'*a*b*', b'a*', b'*b', b'*zz*', b'*a\nb*', b'ab*ab'],
    'icase': [b'a', b'AB', b'zz', b'bA', b'a\nb', b'abab'],
    'icase_all': [[b'a', b'B'], ([b'A'], [b' ']), [b'zz'], [b'aB', b'Ba'], [b'abab']],
    'icase_glob': [b'*a*B*', b'A*', b'*b', b'*zz*', b'AB*ab'],
    'near': ([b'abab', b'aabb', b'zzzz', b'ab', b'a\nbb', b'bbaa'], [1, 1, 1, 0, 1, 2]),
    'edit': ([b'abab', b'aabb', b'zzzz', b'ab', b'a\nbb', b'bbaa'], [1, 1, 1, 0, 1, 2]),
}
REFS = {}


def ref_of(kind, chunks=CHUNKS):
    key = (kind.name, len(chunks))
    if key not in REFS:
        REFS[key] = kind.ref_cls(chunks)
    return REFS[key]


class FakeReader:
    """The Reader calls that check() makes, answered from the kind's reference.  bend_rows(per) may corrupt the ids of the
    rows before anything is made of them (so every call agrees on the corruption); bend(call, answer) may corrupt what
    one call ('ids', 'packed' or 'counts') returns: answer.ids, .counts, .pk and the statistics answer.st."""

    def __init__(self, kind, ref, bend_rows=None, bend=None, result_order='text'):
        self.kind, self.ref, self.bend_rows, self.bend = kind, ref, bend_rows, bend
        self.num_chunks, self.result_order, self.st = len(ref.chunks), result_order, None

    def __getattr__(self, name):        # search_*_ids_batch, search_*_batch_packed, count_*: whatever the kind's calls are named
        call = 'ids' if name.endswith('ids_batch') else 'packed' if name.endswith('_packed') else 'counts' if name.startswith('count_') else None
        if call is None:
            raise AttributeError(name)
        return lambda *args, **kw: self.answer(call, args[0] if len(args) == 1 else args)

    def answer(self, call, batch):
        kind, ref = self.kind, self.ref
        rows = kind.rows(batch)
        live = bool(rows) and self.num_chunks > 0
        per = [np.asarray((kind.ordered or kind.want)(ref, *row), dtype=np.uint64) for row in rows]
        if self.bend_rows:
            self.bend_rows(per)
        a = types.SimpleNamespace(ids=np.concatenate(per + [EMPTY]), counts=np.array([x.size for x in per], dtype=np.uint64))
        a.ids.flags.writeable = False
        a.pk = self.entries_by_id_packed(a.ids)._replace(counts=a.counts)
        route = kind.need | R['INTERVAL_GROUP'] | (R['COUNTS'] if call == 'counts' else 0)
        if kind.plain and self.result_order == 'sa':
            route |= R['SA_ORDER']
        hits = a.ids.size + 3 if kind.want_hits is None else kind.want_hits(ref, batch) if live else 0
        a.st = {'queries': len(rows), 'hits': hits, 'entries': a.ids.size, 'route': route,
                'result_bytes': {'ids': 8 * a.ids.size, 'packed': a.pk.data.size, 'counts': 0}[call]}
        if self.bend:
            self.bend(call, a)
        self.st = a.st
        return {'ids': IdResult(a.ids, a.counts), 'packed': a.pk, 'counts': a.counts.tolist()}[call]

    def last_stats(self):
        return dict(self.st)

    def entries_by_id(self, ids):
        return [self.ref.entry(i) for i in np.asarray(ids).tolist()]

    def entries_by_id_packed(self, ids):
        texts = self.entries_by_id(ids)
        offsets = np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64)
        return PackedResult(np.frombuffer(b''.join(texts), dtype=np.uint8).copy(), offsets, np.ones(len(texts), dtype=np.uint64))


def run(kind, interval=None, **fake):
    return H.check(kind, FakeReader(kind, ref_of(kind), **fake), ref_of(kind), BATCHES[kind.name], interval=interval)


def in_a_row(change):
    """change(ids of the first row that has two or more) -> its corrupted ids, as a bend_rows."""
    def bend_rows(per):
        i = next(i for i, x in enumerate(per) if x.size >= 2)
        per[i] = change(per[i])
    return bend_rows


def on(calls, change):
    """change(answer) on the named calls, as a bend."""
    def bend(call, a):
        if call in calls:
            change(a)
    return bend


def stat(key, change):
    return lambda a: a.st.__setitem__(key, change(a.st[key]))


def data_changed(a):
    a.pk.data[0] ^= 0x20


# what check() must reject: name -> (FakeReader arguments, the kinds it applies to)
EVERY = lambda kind: True
EVERY_CALL = lambda kind: not kind.plain           # plain ids: the routes and statistics of the other two calls are not stated
CORRUPTIONS = {
    'an id dropped': (dict(bend_rows=in_a_row(lambda x: x[1:])), EVERY),
    'an id doubled': (dict(bend_rows=in_a_row(lambda x: np.concatenate([x, x[:1]]))), EVERY),
    'two ids swapped': (dict(bend_rows=in_a_row(lambda x: np.concatenate([x[1::-1], x[2:]]))), lambda kind: kind.ordered is not None),
    'a count off by one': (dict(bend=on(['counts'], lambda a: a.counts.__setitem__(0, a.counts[0] + 1))), EVERY),
    'a packed text changed': (dict(bend=on(['packed'], data_changed)), EVERY),
    'packed offsets shifted': (dict(bend=on(['packed'], lambda a: a.pk.offsets.__iadd__(np.uint64(1)))), EVERY),
    'packed counts of another batch': (dict(bend=on(['packed'], lambda a: a.pk.counts.__setitem__(0, a.pk.counts[0] + 1))), EVERY),
    'hits too many': (dict(bend=on(['ids'], stat('hits', lambda h: h + 1))), lambda kind: kind.want_hits is not None),
    'hits below the ids': (dict(bend=on(['ids'], lambda a: a.st.__setitem__('hits', a.ids.size - 1))), lambda kind: kind.want_hits is None and not kind.plain),
    'hits of the counts call': (dict(bend=on(['counts'], stat('hits', lambda h: h + 1))), EVERY_CALL),
    'hits of the packed call': (dict(bend=on(['packed'], stat('hits', lambda h: h + 1))), EVERY_CALL),
    'entries of the ids call': (dict(bend=on(['ids'], stat('entries', lambda n: n + 1))), EVERY),
    'entries of the counts call': (dict(bend=on(['counts'], stat('entries', lambda n: n - 1))), EVERY_CALL),
    'result_bytes of the ids call': (dict(bend=on(['ids'], stat('result_bytes', lambda n: n + 8))), EVERY),
    'result_bytes of the packed call': (dict(bend=on(['packed'], stat('result_bytes', lambda n: n + 1))), EVERY_CALL),
    'queries': (dict(bend=on(['ids'], stat('queries', lambda n: n + 1))), EVERY),
    'COUNTS on the ids call': (dict(bend=on(['ids'], stat('route', lambda rt: rt | R['COUNTS']))), EVERY),
    'no COUNTS on the counts call': (dict(bend=on(['counts'], stat('route', lambda rt: rt & ~R['COUNTS']))), EVERY_CALL),
    'MID': (dict(bend=on(['ids'], stat('route', lambda rt: rt | R['MID']))), EVERY),
    'SMALL_BLOCK': (dict(bend=on(['ids'], stat('route', lambda rt: rt | R['SMALL_BLOCK']))), EVERY),
    'MID on the packed call': (dict(bend=on(['packed'], stat('route', lambda rt: rt | R['MID']))), EVERY_CALL),
    'ANCHORED': (dict(bend=on(['ids'], stat('route', lambda rt: rt | R['ANCHORED']))), lambda kind: kind is not H.ANCHORED),
    'no ANCHORED': (dict(bend=on(['ids'], stat('route', lambda rt: rt & ~R['ANCHORED']))), lambda kind: kind is H.ANCHORED),
    'no GENERAL': (dict(bend=on(['ids'], stat('route', lambda rt: rt & ~R['GENERAL']))), EVERY),
    'no interval bit': (dict(bend=on(['ids'], stat('route', lambda rt: rt & ~H.INTERVAL))), EVERY_CALL),
    'SA_ORDER': (dict(bend=on(['ids'], stat('route', lambda rt: rt | R['SA_ORDER']))), EVERY),
    'ids writeable': (dict(bend=on(['ids'], lambda a: setattr(a, 'ids', a.ids.copy()))), EVERY),
    'ids of another dtype': (dict(bend=on(['ids'], lambda a: setattr(a, 'ids', a.ids.astype(np.int64)))), EVERY),
}


@pytest.mark.parametrize('kind', H.KINDS, ids=lambda kind: kind.name)
def test_the_honest_reader_passes(kind):
    res = run(kind)
    rows = H.per_row(res)
    assert len(rows) == len(kind.rows(BATCHES[kind.name])) and sum(x.size >= 2 for x in rows) >= 2 and any(x.size == 0 for x in rows)
    if not kind.plain:
        run(kind, interval=R['INTERVAL_GROUP'])
    else:       # order='sa': the SA_ORDER bit follows the reader
        H.check(kind, FakeReader(kind, ref_of(kind), result_order='sa'), ref_of(kind), BATCHES[kind.name])


@pytest.mark.parametrize('kind,what', [(kind, what) for kind in H.KINDS for what, (_, applies) in CORRUPTIONS.items() if applies(kind)],
                         ids=lambda v: getattr(v, 'name', v))
def test_a_corrupted_answer_is_rejected(kind, what):
    with pytest.raises(AssertionError):
        run(kind, **CORRUPTIONS[what][0])


@pytest.mark.parametrize('kind', [kind for kind in H.KINDS if kind.ordered is None], ids=lambda kind: kind.name)
def test_where_no_order_is_stated_swapped_ids_are_the_same_answer(kind):
    run(kind, **CORRUPTIONS['two ids swapped'][0])


@pytest.mark.parametrize('kind', H.KINDS, ids=lambda kind: kind.name)
def test_the_wrong_interval_route_and_the_wrong_result_order_are_rejected(kind):
    if kind.plain:
        with pytest.raises(AssertionError):         # a reader opened with order='sa' whose route lacks SA_ORDER
            H.check(kind, FakeReader(kind, ref_of(kind), result_order='sa', bend=on(['ids'], stat('route', lambda rt: rt & ~R['SA_ORDER']))),
                    ref_of(kind), BATCHES[kind.name])
        run(kind, interval=R['INTERVAL_WAVE'])      # nothing is stated about the interval bit of a plain ids batch
    else:
        for call in ('ids', 'counts', 'packed'):
            with pytest.raises(AssertionError):
                run(kind, interval=R['INTERVAL_GROUP'], bend=on([call], stat('route', lambda rt: rt & ~H.INTERVAL | R['INTERVAL_LANE'])))
        with pytest.raises(AssertionError):
            run(kind, interval=R['INTERVAL_WAVE'])


@pytest.mark.parametrize('kind', H.KINDS, ids=lambda kind: kind.name)
def test_an_empty_batch_and_a_reader_without_chunks_assert_no_route(kind):
    """`live` is false: whatever the route word says, nothing is asserted about it."""
    batch = BATCHES[kind.name]
    empty = ([], batch[1][:0]) if isinstance(batch, tuple) else []
    no_route = on(['ids', 'counts', 'packed'], stat('route', lambda rt: 0))
    res = H.check(kind, FakeReader(kind, ref_of(kind), bend=no_route), ref_of(kind), empty)
    assert res.ids.size == 0 and res.counts.size == 0
    none = ref_of(kind, [])
    res = H.check(kind, FakeReader(kind, none, bend=no_route), none, batch)
    assert res.ids.size == 0 and res.counts.tolist() == [0] * len(kind.rows(batch))
