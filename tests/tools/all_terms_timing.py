"""The all-terms search next to ids + numpy set operations on the same groups (MI355X; run by hand, not by the suite):

    python tests/tools/all_terms_timing.py [--commit HASH] [--out profiles/all_terms_vs_ids.json]

One 64 MiB chunk of `words` text (pss_gen_corpus), its suffix array by pss_sa_build, handed to a reader on the device.
The groups pair a FREQUENT term with a RARE one, in both orders: the `--pairs` most frequent words of a sample of the text
(each in a large share of the entries) against as many words that occur a handful of times, [frequent, rare] and
[rare, frequent] for every pair.  Two legs on those groups, on the same reader:
    all_terms   search_all_ids_batch(groups): one device call, the rarest term of every group drives;
    ids_numpy   search_ids_batch(distinct terms), then np.intersect1d per group on the host: what the README recommended
                before the device call existed.  Every id of every term comes through the pipeline and over PCIe.
Before anything is timed the two legs' answers are compared group by group (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg (every library call ends in a stream synchronise); the legs
alternate for `--rounds` rounds, so the spread between two runs of the same leg is on record next to the difference
between the legs.  Reported: median / min / max per leg and round, hits and device time of the leg's last library
call (last_stats), and the ratio of the medians.  No threshold: a record, not a test."""
import json
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_terms, time_legs, words_reader, write_json


def main():
    args = arguments('all_terms_vs_ids.json', ('--pairs', 16))
    r, text, _ = words_reader(close=False)
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    groups = []
    for f, x in zip(frequent, rare):
        groups += [[f, x], [x, f]]
    terms = sorted(set(frequent + rare))
    term_at = {t: i for i, t in enumerate(terms)}

    def all_terms():
        return per_row(r.search_all_ids_batch(groups))

    def ids_numpy():
        per = per_row(r.search_ids_batch(terms))
        return [np.intersect1d(per[term_at[a]], per[term_at[b]], assume_unique=True) for a, b in groups]

    a, b = all_terms(), ids_numpy()
    for g, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(np.sort(x), y):
            raise SystemExit(f'group {g} {groups[g]}: the two legs disagree ({x.size} against {y.size} ids)')
    term_entries = {t.decode('latin-1'): int(c) for t, c in zip(terms, r.search_ids_batch(terms).counts)}

    def record(out, st):
        return {'entries': int(sum(x.size for x in out)), 'hits_last_call': int(st['hits']), 'entries_last_call': int(st['entries']),
                'result_bytes_last_call': int(st['result_bytes']), 'ms_device_last_call': round(st['ms_device'], 4),
                'ms_interval_last_call': round(st['ms_interval'], 4), 'route': hex(st['route'])}

    legs = {'all_terms': all_terms, 'ids_numpy': ids_numpy}
    runs = time_legs(legs, lambda name: r.last_stats(), args.warmup, args.reps, args.rounds, record)
    r.close()
    summary = medians(runs, legs)
    ratio = statistics.median(summary['ids_numpy']) / statistics.median(summary['all_terms'])
    out = {'what': 'search_all_ids_batch(groups) vs search_ids_batch(distinct terms) + np.intersect1d per group, same reader: one 64 MiB chunk '
                   'of `words`, groups [frequent word, rare word] and [rare, frequent]; host clock around the whole leg (every library call '
                   'ends in a stream synchronise; packing the batch in Python and the numpy set operations included), median / min / max '
                   'over reps after warm-up; the two legs alternate; the answers were compared group by group before the timing',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'groups': len(groups), 'distinct_terms': len(terms),
           'entries_per_term': term_entries, 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'ids_numpy_over_all_terms': round(ratio, 2)}
    write_json(out, args.out)
    print(json.dumps({'summary': summary, 'ids_numpy_over_all_terms': out['ids_numpy_over_all_terms']}))


if __name__ == '__main__':
    main()
