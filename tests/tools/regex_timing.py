"""The regular-expression search next to the route that existed before it, on the same patterns (MI355X; run by hand, not by
the suite):

    python tests/tools/regex_timing.py [--commit HASH] [--out profiles/regex_vs_host_filter.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device -- the reader of tests/tools/glob_timing.py.  The patterns pair a RARE word with a FREQUENT one around
an alternation and a counted class: `RARE.{0,12}(FREQUENT|zzzz)` and `FREQUENT\\W+(\\w+\\W+){0,3}RARE`, 2 x --pairs of them.  Two
legs on those patterns, on the same reader:
    regex         search_regex_ids_batch(patterns): the batch is compiled (ms_compile says what that costs, measured apart
                  with regex_info over the same patterns), the rarest required literal drives, every candidate is walked
                  through its DFA on the device;
    host_filter   search_all_ids_batch over regex_literals of every pattern, entries_by_id_packed(ids), Python's `re` over
                  every candidate's text, then indexing the ids.
Before anything is timed the two legs' answers are compared pattern by pattern (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg; the legs alternate for `--rounds` rounds.  Reported: median /
min / max per leg and round, hits and device time (last_stats) of the leg's search call, and the ratio of the medians.
Last, ONE batch whose driver is frequent is timed as it is: `FREQUENT [a-z]+ [a-z]+ing`, whose literals are one of the most
frequent words and `ing`, so whichever drives has many hits and every entry that holds both is a candidate walked by ONE
LANE -- where one lane per entry shows.  No host-filter leg stands beside it (every candidate would cross PCIe).  Not timed: long entries (`words`
entries are short) and several chunks.  No threshold: a record, not a test."""
import json
import re
import statistics
import time

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_terms, search_call_record, time_legs, words_reader, write_json


def main():
    args = arguments('regex_vs_host_filter.json', ('--pairs', 16))
    r, text, _ = words_reader()
    from pysubstringsearch_amd import regex_escape, regex_info, regex_literals
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    patterns = []
    for f, x in zip(frequent, rare):
        f, x = regex_escape(f), regex_escape(x)
        patterns += [x + b'.{0,12}(' + f + b'|zzzz)', f + rb'\W+(\w+\W+){0,3}' + x]
    groups = [(regex_literals(p), []) for p in patterns]
    filters = [re.compile(p) for p in patterns]
    compile_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        states = [regex_info(p)['states'] for p in patterns]
        compile_ms.append((time.perf_counter() - t0) * 1e3)
    out = {'what': 'search_regex_ids_batch(patterns) vs search_all_ids_batch over regex_literals + entries_by_id_packed + Python `re` over every '
                   'candidate + indexing the ids, same reader: one 64 MiB chunk of `words`, patterns RARE.{0,12}(FREQUENT|zzzz) and '
                   'FREQUENT\\W+(\\w+\\W+){0,3}RARE; host clock around the whole leg (packing and compiling the batch and the host filter included), '
                   'median / min / max over reps after warm-up; the two legs alternate; the answers were compared pattern by pattern before the '
                   'timing; ms_device is last_stats() of the leg\'s search call; ms_compile is regex_info over every pattern of the batch, '
                   'measured apart (the search call compiles the batch again, every time); then the frequent-driver batch, the device call alone',
           'commit': args.commit or commit_hash(), 'chunk_bytes': int(text.size), 'patterns': len(patterns), 'warmup': args.warmup, 'reps': args.reps,
           'dfa_states': {'min': min(states), 'max': max(states)}, 'ms_compile': round(statistics.median(compile_ms), 4),
           'not_timed': ['entries longer than the `words` corpus has', 'more than one chunk', 'a host-filter leg beside the frequent-driver batch',
                         'icase=True']}
    seen = {}

    def regex():
        res = r.search_regex_ids_batch(patterns)
        seen['regex'] = r.last_stats()
        return per_row(res)

    def host_filter():
        res = r.search_all_ids_batch(groups)
        seen['host_filter'] = r.last_stats()
        pk = r.entries_by_id_packed(res.ids)
        data, o = pk.data.tobytes(), pk.offsets.tolist()
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64)))).tolist()
        kept = []
        for g, rx in enumerate(filters):
            keep = [i for i in range(bounds[g], bounds[g + 1]) if rx.search(data, o[i], o[i + 1])]
            kept.append(res.ids[keep])
        return kept

    a, b = regex(), host_filter()
    for g, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(np.sort(x), np.sort(y)):
            raise SystemExit(f'pattern {g} {patterns[g]}: the two legs disagree ({x.size} against {y.size} ids)')
    candidates = int(r.search_all_ids_batch(groups).ids.size)

    def record(got, st):
        rec = search_call_record(got, st)
        del rec['queries_search_call']
        return rec

    legs = {'regex': regex, 'host_filter': host_filter}
    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds, record)
    summary = medians(runs, legs)
    ratio = statistics.median(summary['host_filter']) / statistics.median(summary['regex'])
    out['exact'] = {'candidates_all_terms': candidates, 'entries_regex': int(sum(x.size for x in a)), 'runs': runs, 'summary': summary,
                    'host_filter_over_regex': round(ratio, 2)}
    # a frequent driver: the literals of every pattern are one of the most frequent words and `ing`
    heavy = [regex_escape(f) + b' [a-z]+ [a-z]+ing' for f in frequent[:8]]
    seen = {}

    def frequent_driver():
        res = r.search_regex_ids_batch(heavy)
        seen['frequent_driver'] = r.last_stats()
        return per_row(res)

    runs = time_legs({'frequent_driver': frequent_driver}, seen, args.warmup, args.reps, args.rounds)
    out['frequent_driver'] = {'patterns': [p.decode('latin-1') for p in heavy], 'literals': [[x.decode('latin-1') for x in regex_literals(p)] for p in heavy],
                              'runs': runs}
    r.close()
    write_json(out, args.out)
    print(json.dumps({'exact': out['exact']['summary'], 'ratio_exact': out['exact']['host_filter_over_regex'], 'ms_compile': out['ms_compile'],
                      'frequent_driver': [(x['median_ms'], x['hits_search_call'], x['entries'], x['ms_device_search_call']) for x in runs]}))


if __name__ == '__main__':
    main()
