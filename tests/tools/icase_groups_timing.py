"""The case-insensitive all-terms and wildcard search next to what the engine offered for the same answers before them
(MI355X; run by hand, not by the suite):

    python tests/tools/icase_groups_timing.py [--commit HASH] [--out profiles/icase_groups_vs_host.json]

One 64 MiB chunk of `words` text, case-mangled as in tests/tools/icase_timing.py (about 1/8 of the words capitalised, about
1/32 upper-cased), its suffix array by pss_sa_build, handed to a reader on the device.  32 pairs of a FREQUENT and a RARE
word of 4 .. 10 letters from the text's frequency ranking.  The legs, on the same reader:
    all_device    search_all_ids_batch(groups, icase=True), group g = [frequent_g, RARE_g]: one device call;
    all_host      the route before: search_icase_ids_batch over the 64 terms in one call, then np.intersect1d per group on
                  the host;
    glob_device   search_glob_ids_batch(patterns, icase=True), patterns `*FREQUENT*RARE*` and `*RARE*FREQUENT*` in turn:
                  one device call;
    glob_host     search_all_ids_batch(groups, icase=True) for the candidates, entries_by_id_packed for their text, then
                  Python's re with re.IGNORECASE over every candidate of every pattern.
Before anything is timed the device legs' answers are compared with the host legs' row by row (sorted ids).  Each leg is
warmed up, then timed `--reps` times with a host clock around the whole leg (every library call ends in a stream
synchronise); the legs alternate for `--rounds` rounds.  Reported: median / min / max per leg and round, the spread of the
medians across the rounds, hits against entries and the device time (last_stats) of the leg's last search call.  No
threshold: a record, not a test."""
import collections
import json
import re
import statistics

import numpy as np

from icase_timing import mangle_words
from timing_common import arguments, commit_hash, medians, per_row, time_legs, words_reader, write_json


def pick_pairs(text: bytes, count: int):
    """`count` (frequent, rare) pairs of alphabetic words of 4 .. 10 letters, lower case: the frequent ones from the top of
    the frequency ranking of the first 4 MiB, the rare ones from ranks 1000 .. 2000."""
    words = collections.Counter(text[:4 << 20].lower().replace(b'\n', b' ').split(b' '))
    ranked = [w for w, _ in words.most_common() if 4 <= len(w) <= 10 and w.isalpha()]
    if len(ranked) < 2000:
        raise SystemExit(f'the corpus yields {len(ranked)} words of 4 .. 10 letters, 2000 are wanted')
    return [(ranked[i], ranked[1000 + i * 1000 // count]) for i in range(count)]


def main():
    args = arguments('icase_groups_vs_host.json', ('--groups', 32))
    r, text, _ = words_reader(edit=lambda t: mangle_words(t, np.random.default_rng(20)))
    pairs = pick_pairs(text.tobytes(), args.groups)
    groups = [[f, x.upper()] for f, x in pairs]
    terms = [t for g in groups for t in g]
    order = [(f.upper(), x) if g % 2 == 0 else (x.upper(), f) for g, (f, x) in enumerate(pairs)]
    globs = [b'*' + a + b'*' + b + b'*' for a, b in order]
    regexes = [re.compile(b'.*' + re.escape(a) + b'.*' + re.escape(b) + b'.*', re.IGNORECASE | re.DOTALL) for a, b in order]
    seen = {}

    def all_device():
        res = r.search_all_ids_batch(groups, icase=True)
        seen['all_device'] = r.last_stats()
        return per_row(res)

    def all_host():
        res = r.search_icase_ids_batch(terms)
        seen['all_host'] = r.last_stats()
        rows = per_row(res)
        return [np.intersect1d(rows[2 * g], rows[2 * g + 1]) for g in range(len(groups))]

    def glob_device():
        res = r.search_glob_ids_batch(globs, icase=True)
        seen['glob_device'] = r.last_stats()
        return per_row(res)

    def glob_host():
        res = r.search_all_ids_batch(groups, icase=True)
        seen['glob_host'] = r.last_stats()
        pk = r.entries_by_id_packed(res.ids)
        data, o = pk.data.tobytes(), pk.offsets.tolist()
        b = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64)))).tolist()
        out = []
        for g, rx in enumerate(regexes):
            keep = [i for i in range(b[g], b[g + 1]) if rx.fullmatch(data, o[i], o[i + 1])]
            out.append(res.ids[keep])
        return out

    legs = {'all_device': all_device, 'all_host': all_host, 'glob_device': glob_device, 'glob_host': glob_host}
    for dev, host in (('all_device', 'all_host'), ('glob_device', 'glob_host')):
        for g, (x, y) in enumerate(zip(legs[dev](), legs[host]())):
            if not np.array_equal(np.sort(x), np.sort(y)):
                raise SystemExit(f'{dev}, row {g}: {x.size} ids against {y.size} of {host}')

    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds)
    r.close()
    summary = medians(runs, legs)
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_all_ids_batch(groups, icase=True), 32 groups [frequent, RARE], vs search_icase_ids_batch over the 64 terms + '
                   'np.intersect1d per group on the host; search_glob_ids_batch(patterns, icase=True), 32 patterns *FREQUENT*RARE* / '
                   '*RARE*FREQUENT*, vs the all-terms ids under fold + entries_by_id_packed + re.IGNORECASE on the host; same reader: one '
                   '64 MiB chunk of `words`, about 1/8 of the words capitalised and 1/32 upper-cased; host clock around the whole leg '
                   '(packing the batch in Python and the host-side work included), median / min / max over reps after warm-up; the legs '
                   'alternate; the device answers were compared with the host legs row by row before the timing; hits / entries / '
                   'ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'pairs': [[f.decode(), x.decode()] for f, x in pairs],
           'warmup': args.warmup, 'reps': args.reps, 'rounds': args.rounds, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'spread_of_medians_ms': {k: [round(min(v), 4), round(max(v), 4)] for k, v in summary.items()},
           'all_host_over_all_device': round(med['all_host'] / med['all_device'], 2),
           'glob_host_over_glob_device': round(med['glob_host'] / med['glob_device'], 2)}
    write_json(out, args.out)
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'spread_of_medians_ms': out['spread_of_medians_ms'],
                      'all_host_over_all_device': out['all_host_over_all_device'],
                      'glob_host_over_glob_device': out['glob_host_over_glob_device']}))


if __name__ == '__main__':
    main()
