"""The search within k mismatches next to the route that existed before it, on the same patterns (MI355X; run by hand, not by
the suite):

    python tests/tools/near_timing.py [--commit HASH] [--out profiles/near_vs_variants.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  32 patterns of 8 .. 12 letters, words of the text spread over its frequency ranking.  The legs, on
the same reader:
    near_k1        search_near_ids_batch(patterns, 1): one device call;
    variants_k1    the route the engine had before: every one-substitution variant of every pattern over the bytes that
                   occur in the corpus (0x0A left out: such a variant matches nothing), and the pattern itself, through
                   search_ids_batch, then np.unique over each pattern's ids on the host -- L * (A - 1) + 1 patterns each;
    plain          the patterns themselves through search_ids_batch: the floor (it answers another question);
    near_k2        search_near_ids_batch(patterns, 2), timed against itself only: its enumeration is quadratic, and only the
                   number of variants it would take is written down.
Before anything is timed near_k1's answers are compared with variants_k1's pattern by pattern (sorted ids).  Each leg is
warmed up, then timed `--reps` times with a host clock around the whole leg (every library call ends in a stream
synchronise); the legs alternate for `--rounds` rounds.  Reported: median / min / max per leg and round, hits against
entries and the device time (last_stats) of the leg's last search call.  No threshold: a record, not a test."""
import json
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_patterns, time_legs, words_reader, write_json


def variants(word: bytes, alphabet: bytes):
    """The word and every word one substitution away over the alphabet."""
    out = [word]
    for i, b in enumerate(word):
        out += [word[:i] + bytes([x]) + word[i + 1:] for x in alphabet if x != b]
    return out


def main():
    args = arguments('near_vs_variants.json', ('--patterns', 32))
    r, text, alphabet = words_reader()
    patterns = pick_patterns(text.tobytes(), args.patterns)
    every = [variants(p, alphabet) for p in patterns]
    flat = [s for group in every for s in group]
    bounds_q = np.concatenate(([0], np.cumsum([len(g) for g in every])))
    a1 = len(alphabet) - 1
    variants_k2 = sum(1 + len(p) * a1 + len(p) * (len(p) - 1) // 2 * a1 * a1 for p in patterns)
    seen = {}

    def near(k):
        def leg():
            res = r.search_near_ids_batch(patterns, k)
            seen[f'near_k{k}'] = r.last_stats()
            return per_row(res)
        return leg

    def variants_k1():
        res = r.search_ids_batch(flat)
        seen['variants_k1'] = r.last_stats()
        rows = per_row(res)
        return [np.unique(np.concatenate(rows[bounds_q[g]:bounds_q[g + 1]])) for g in range(len(patterns))]

    def plain():
        res = r.search_ids_batch(patterns)
        seen['plain'] = r.last_stats()
        return per_row(res)

    legs = {'near_k1': near(1), 'variants_k1': variants_k1, 'plain': plain, 'near_k2': near(2)}
    want = variants_k1()
    for g, (x, y) in enumerate(zip(legs['near_k1'](), want)):
        if not np.array_equal(np.sort(x), y):
            raise SystemExit(f'near_k1, pattern {g} {patterns[g]}: {x.size} ids against {y.size} of the variants')

    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds)
    r.close()
    summary = medians(runs, legs)
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_near_ids_batch(patterns, 1) vs every one-substitution variant of every pattern over the bytes of the corpus '
                   'through search_ids_batch + np.unique per pattern (the route before), vs the patterns through search_ids_batch (the '
                   'floor), and search_near_ids_batch(patterns, 2) against itself; same reader: one 64 MiB chunk of `words`; host clock '
                   'around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over reps '
                   'after warm-up; the legs alternate; the near_k1 answers were compared with variants_k1 pattern by pattern before the '
                   'timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'patterns': [p.decode() for p in patterns],
           'alphabet_bytes': len(alphabet), 'variants_k1_total': len(flat), 'variants_k2_total_not_run': variants_k2,
           'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'variants_k1_over_near_k1': round(med['variants_k1'] / med['near_k1'], 2),
           'near_k1_over_plain': round(med['near_k1'] / med['plain'], 2)}
    write_json(out, args.out)
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'variants_k1_over_near_k1': out['variants_k1_over_near_k1']}))


if __name__ == '__main__':
    main()
