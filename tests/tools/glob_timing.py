"""The wildcard search next to the route that existed before it, on the same patterns (MI355X; run by hand, not by the suite):

    python tests/tools/glob_timing.py [--commit HASH] [--out profiles/glob_vs_host_filter.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  The patterns pair a FREQUENT word with a RARE one, in both orders: `*FREQUENT*RARE*` and
`*RARE*FREQUENT*` for each of `--pairs` pairs (the words are picked as tests/tools/all_terms_timing.py picks them).  Two
legs on those patterns, on the same reader:
    glob          search_glob_ids_batch(patterns): one device call, the rarest segment drives, the order is verified on
                  the device;
    host_filter   search_all_ids_batch([[f, x]] per pattern), entries_by_id_packed(ids), a Python `re` over every
                  candidate's text on the host, then indexing the ids: every candidate's text crosses PCIe.
Before anything is timed the two legs' answers are compared pattern by pattern (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg (every library call ends in a stream synchronise); the legs
alternate for `--rounds` rounds, so the spread between two runs of the same leg is on record next to the difference
between the legs.  Reported: median / min / max per leg and round, hits and device time (last_stats) of the leg's search
call, and the ratio of the medians.  No threshold: a record, not a test.  With rare words for drivers the candidates are
few, so this says what the two extra trips cost on a small answer -- and nothing about the verify kernel's shape: 8 lanes
against one lane per candidate stays unmeasured."""
import json
import re
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_terms, search_call_record, time_legs, words_reader, write_json


def main():
    args = arguments('glob_vs_host_filter.json', ('--pairs', 16))
    r, text, _ = words_reader()         # (every entry closed: the text handed out by id is then every entry's whole text)
    from pysubstringsearch_amd import glob_escape
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    segs = []
    for f, x in zip(frequent, rare):
        segs += [(f, x), (x, f)]
    patterns = [b'*' + glob_escape(a) + b'*' + glob_escape(b) + b'*' for a, b in segs]
    groups = [[a, b] for a, b in segs]
    filters = [re.compile(b'.*' + re.escape(a) + b'.*' + re.escape(b) + b'.*', re.DOTALL) for a, b in segs]
    seen = {}

    def glob():
        res = r.search_glob_ids_batch(patterns)
        seen['glob'] = r.last_stats()
        return per_row(res)

    def host_filter():
        res = r.search_all_ids_batch(groups)
        seen['host_filter'] = r.last_stats()
        pk = r.entries_by_id_packed(res.ids)
        data, o = pk.data.tobytes(), pk.offsets.tolist()
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64)))).tolist()
        out = []
        for g, rx in enumerate(filters):
            keep = [i for i in range(bounds[g], bounds[g + 1]) if rx.fullmatch(data, o[i], o[i + 1])]
            out.append(res.ids[keep])
        return out

    a, b = glob(), host_filter()
    for g, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(np.sort(x), np.sort(y)):
            raise SystemExit(f'pattern {g} {patterns[g]}: the two legs disagree ({x.size} against {y.size} ids)')
    candidates = int(r.search_all_ids_batch(groups).ids.size)

    def record(out, st):
        rec = search_call_record(out, st)
        del rec['queries_search_call']
        return rec

    legs = {'glob': glob, 'host_filter': host_filter}
    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds, record)
    r.close()
    summary = medians(runs, legs)
    ratio = statistics.median(summary['host_filter']) / statistics.median(summary['glob'])
    out = {'what': 'search_glob_ids_batch(patterns) vs search_all_ids_batch + entries_by_id_packed + a host `re` over every candidate + '
                   'indexing the ids, same reader: one 64 MiB chunk of `words`, patterns *FREQUENT*RARE* and *RARE*FREQUENT*; host clock '
                   'around the whole leg (every library call ends in a stream synchronise; packing the batch in Python and the host filter '
                   'included), median / min / max over reps after warm-up; the two legs alternate; the answers were compared pattern by '
                   'pattern before the timing; ms_device is last_stats() of the leg\'s search call (the glob call, the all-terms call)',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'patterns': len(patterns), 'candidates_all_terms': candidates,
           'entries_glob': int(sum(x.size for x in a)), 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'host_filter_over_glob': round(ratio, 2)}
    write_json(out, args.out)
    print(json.dumps({'summary': summary, 'host_filter_over_glob': out['host_filter_over_glob']}))


if __name__ == '__main__':
    main()
