"""The wildcard search with byte classes next to the route that existed before it, on the same patterns (MI355X; run by hand,
not by the suite):

    python tests/tools/glob_class_timing.py [--commit HASH] [--out profiles/glob_class_vs_host_filter.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  The patterns pair a FREQUENT word with a RARE one as tests/tools/glob_timing.py does, with some
letters replaced: the frequent word's second letter by `?`, the rare word's third by a set of two bytes and its last by a
negated set; every second pattern puts the rare word first and a coreless `??` piece between the two.  Two legs on those
patterns, on the same reader, exact and then again under icase=True:
    glob_class    search_glob_ids_batch(patterns, classes=True): one device call, the rarest core drives, the class
                  positions and the order are verified on the device;
    host_filter   search_all_ids_batch over the cores (glob_cores) of every pattern, entries_by_id_packed(ids), a Python
                  `re` with every position as an explicit byte set over every candidate's text, then indexing the ids.
Before anything is timed the two legs' answers are compared pattern by pattern (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg; the legs alternate for `--rounds` rounds.  Reported: median /
min / max per leg and round, hits and device time (last_stats) of the leg's search call, and the ratio of the medians.
Last, ONE batch that is the retry loop's worst case is timed once per round, as it is: the most frequent words with a
class position behind them that no entry satisfies, so the frequent core drives and every occurrence of it in every
candidate entry fails its class position.  No host-filter leg stands beside it (every entry of the chunk would cross
PCIe), and nothing here says how the walk does on long entries: `words` entries are short.  No threshold: a record, not a
test."""
import json
import re
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_terms, search_call_record, time_legs, words_reader, write_json


def position_regex(members: bytes) -> bytes:
    return b'[' + b''.join(b'\\x%02x' % b for b in members) + b']'


def pattern_regex(pattern: bytes, fold: bool):
    from pysubstringsearch_amd import glob_parse
    segs, anchors = glob_parse(pattern, classes=True, fold=fold)
    body = rb'[^\n]*'.join(b''.join(position_regex(pos) for pos in seg) for seg in segs)
    return re.compile((b'' if anchors & 1 else rb'[^\n]*') + body + (b'' if anchors & 2 else rb'[^\n]*'), re.DOTALL | (re.IGNORECASE if fold else 0))


def classed(word: bytes, at: int, what: bytes) -> bytes:
    from pysubstringsearch_amd import glob_escape
    return glob_escape(word[:at], classes=True) + what + glob_escape(word[at + 1:], classes=True)


def main():
    args = arguments('glob_class_vs_host_filter.json', ('--pairs', 16))
    r, text, _ = words_reader()
    from pysubstringsearch_amd import glob_cores, glob_escape
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    patterns = []
    for k, (f, x) in enumerate(zip(frequent, rare)):
        fq = classed(f, 1, b'?') if len(f) > 2 else glob_escape(f, classes=True) + b'?'
        rx = glob_escape(x[:2], classes=True) + b'[\\' + x[2:3] + b'~]' + glob_escape(x[3:-1], classes=True) + b'[!~]'
        patterns += [b'*' + fq + b'*' + rx + b'*', b'*' + rx + b'*??*' + fq + b'*']
    groups = [[c[1] for c in glob_cores(p) if c is not None] for p in patterns]
    out = {'what': 'search_glob_ids_batch(patterns, classes=True) vs search_all_ids_batch over the cores + entries_by_id_packed + a host `re` '
                   'over every candidate + indexing the ids, same reader: one 64 MiB chunk of `words`, patterns *F?EQUENT*RA[R~]E[!~]* and '
                   '*RA[R~]E[!~]*??*F?EQUENT*; host clock around the whole leg (packing the batch in Python and the host filter included), '
                   'median / min / max over reps after warm-up; the two legs alternate; the answers were compared pattern by pattern before '
                   'the timing; ms_device is last_stats() of the leg\'s search call; then the same under icase=True; then the retry worst '
                   'case, the device call alone',
           'commit': args.commit or commit_hash(), 'chunk_bytes': int(text.size), 'patterns': len(patterns), 'warmup': args.warmup, 'reps': args.reps,
           'not_timed': ['a host-filter leg beside the retry worst case', 'entries longer than the `words` corpus has', 'more than one chunk',
                         '8 lanes against one lane per candidate']}
    for fold in (False, True):
        filters = [pattern_regex(p, fold) for p in patterns]
        seen = {}

        def glob_class():
            res = r.search_glob_ids_batch(patterns, classes=True, icase=fold)
            seen['glob_class'] = r.last_stats()
            return per_row(res)

        def host_filter():
            res = r.search_all_ids_batch(groups, icase=fold)
            seen['host_filter'] = r.last_stats()
            pk = r.entries_by_id_packed(res.ids)
            data, o = pk.data.tobytes(), pk.offsets.tolist()
            bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64)))).tolist()
            kept = []
            for g, rx in enumerate(filters):
                keep = [i for i in range(bounds[g], bounds[g + 1]) if rx.fullmatch(data, o[i], o[i + 1])]
                kept.append(res.ids[keep])
            return kept

        a, b = glob_class(), host_filter()
        for g, (x, y) in enumerate(zip(a, b)):
            if not np.array_equal(np.sort(x), np.sort(y)):
                raise SystemExit(f'pattern {g} {patterns[g]} (icase={fold}): the two legs disagree ({x.size} against {y.size} ids)')
        candidates = int(r.search_all_ids_batch(groups, icase=fold).ids.size)

        def record(got, st):
            rec = search_call_record(got, st)
            del rec['queries_search_call']
            return rec

        legs = {'glob_class': glob_class, 'host_filter': host_filter}
        runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds, record)
        summary = medians(runs, legs)
        ratio = statistics.median(summary['host_filter']) / statistics.median(summary['glob_class'])
        out['icase' if fold else 'exact'] = {'candidates_all_terms': candidates, 'entries_glob_class': int(sum(x.size for x in a)), 'runs': runs,
                                             'summary': summary, 'host_filter_over_glob_class': round(ratio, 2)}
    # the retry loop's worst case: the frequent core drives, and no occurrence of it passes its class position
    worst = [b'*' + glob_escape(f, classes=True) + b'[~^]?*' for f in frequent[:8]]
    seen = {}

    def retry():
        res = r.search_glob_ids_batch(worst, classes=True)
        seen['retry_worst_case'] = r.last_stats()
        return per_row(res)

    runs = time_legs({'retry_worst_case': retry}, seen, args.warmup, 1, args.rounds)
    out['retry_worst_case'] = {'patterns': [p.decode('latin-1') for p in worst], 'runs': runs}
    r.close()
    write_json(out, args.out)
    print(json.dumps({k: out[k].get('summary', out[k].get('runs')) for k in ('exact', 'icase', 'retry_worst_case')}
                     | {'ratio_exact': out['exact']['host_filter_over_glob_class'], 'ratio_icase': out['icase']['host_filter_over_glob_class']}))


if __name__ == '__main__':
    main()
