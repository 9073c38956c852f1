"""The any-of search next to the route that existed before it, on the same sets (MI355X; run by hand, not by the suite):

    python tests/tools/any_timing.py [--commit HASH] [--out profiles/any_vs_host_union.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device -- the reader of the other timing tools.  --sets sets of four words, two FREQUENT and two RARE each
(pick_terms), in exact bytes and with icase=True.  Two legs per form, on the same reader:
    any          search_any_ids_batch(sets): one device call; a set is one term, its alternatives its queries, the dedupe
                 keeps every entry's leftmost match;
    host_union   search_ids_batch (icase: search_icase_ids_batch) over all 4 x --sets words, then per set
                 np.unique(np.concatenate(its four rows)): every hit of every word comes down as 8 bytes.
Before anything is timed the two legs' answers are compared set by set (sorted ids).  Each leg is warmed up, then timed
`--reps` times with a host clock around the whole leg; the legs alternate for `--rounds` rounds.  Reported: median / min /
max per leg and round, hits and device time (last_stats) of the leg's search call, and the ratio of the medians.  Last, ONE
batch of frequent-only sets is timed as it is, in both forms: every entry holds several alternatives several times, so the
dedupe scans the most there.  Not timed: several chunks, sets at the cap.  No threshold: a record, not a test."""
import json
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_terms, time_legs, words_reader, write_json


def main():
    args = arguments('any_vs_host_union.json', ('--sets', 32))
    r, text, _ = words_reader()
    frequent, rare = pick_terms(text.tobytes(), 2 * args.sets)
    sets = [[frequent[2 * g], rare[2 * g], frequent[2 * g + 1], rare[2 * g + 1]] for g in range(args.sets)]
    flat = [w for s in sets for w in s]
    out = {'what': 'search_any_ids_batch(sets) vs search_ids_batch (icase: search_icase_ids_batch) over every word of every set + '
                   'np.unique(np.concatenate(rows)) per set, same reader: one 64 MiB chunk of `words`, sets of two frequent and two rare '
                   'words; host clock around the whole leg (packing the batch and the host union included), median / min / max over reps '
                   'after warm-up; the two legs alternate; the answers were compared set by set before the timing; ms_device is '
                   'last_stats() of the leg\'s search call; then one batch of frequent-only sets, the device call alone',
           'commit': args.commit or commit_hash(), 'chunk_bytes': int(text.size), 'sets': len(sets), 'words': len(flat), 'warmup': args.warmup,
           'reps': args.reps, 'not_timed': ['more than one chunk', 'sets of 64 (32) alternatives', 'a host-union leg beside the frequent-only batch']}
    for form, icase in (('exact', False), ('icase', True)):
        seen = {}

        def any_of():
            res = r.search_any_ids_batch(sets, icase=icase)
            seen['any'] = r.last_stats()
            return per_row(res)

        def host_union():
            res = r.search_icase_ids_batch(flat) if icase else r.search_ids_batch(flat)
            seen['host_union'] = r.last_stats()
            rows = per_row(res)
            return [np.unique(np.concatenate(rows[4 * g:4 * g + 4])) for g in range(len(sets))]

        a, b = any_of(), host_union()
        for g, (x, y) in enumerate(zip(a, b)):
            if not np.array_equal(np.sort(x), y):
                raise SystemExit(f'{form}, set {g} {sets[g]}: the two legs disagree ({x.size} against {y.size} ids)')
        legs = {'any': any_of, 'host_union': host_union}
        runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds)
        summary = medians(runs, legs)
        ratio = statistics.median(summary['host_union']) / statistics.median(summary['any'])
        out[form] = {'entries_any': int(sum(x.size for x in a)), 'runs': runs, 'summary': summary, 'host_union_over_any': round(ratio, 2)}
    heavy = [frequent[4 * g:4 * g + 4] for g in range(min(8, len(frequent) // 4))]
    out['frequent_only'] = {'sets': [[w.decode('latin-1') for w in s] for s in heavy]}
    for form, icase in (('exact', False), ('icase', True)):
        seen = {}

        def frequent_only():
            res = r.search_any_ids_batch(heavy, icase=icase)
            seen['frequent_only'] = r.last_stats()
            return per_row(res)

        out['frequent_only'][form] = time_legs({'frequent_only': frequent_only}, seen, args.warmup, args.reps, args.rounds)
    r.close()
    write_json(out, args.out)
    print(json.dumps({form: {'summary': out[form]['summary'], 'ratio': out[form]['host_union_over_any']} for form in ('exact', 'icase')} |
                     {'frequent_only': {form: [(x['median_ms'], x['hits_search_call'], x['entries'], x['ms_device_search_call'])
                                               for x in out['frequent_only'][form]] for form in ('exact', 'icase')}}))


if __name__ == '__main__':
    main()
