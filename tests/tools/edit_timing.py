"""The search within k edits next to the route that existed before it and next to the search within k mismatches, on the same
patterns (MI355X; run by hand, not by the suite):

    python tests/tools/edit_timing.py [--commit HASH] [--out profiles/edit_vs_variants.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  32 patterns of 8 .. 12 letters, words of the text spread over its frequency ranking (the patterns of
tests/tools/near_timing.py).  The legs, on the same reader:
    edit_k1        search_near_ids_batch(patterns, 1, edits=True): one device call;
    variants_k1    the route the engine had before: every string within one edit of every pattern over the bytes that occur
                   in the corpus (0x0A left out: such a variant matches nothing) -- substitutions, insertions, deletions and
                   the pattern itself --, through search_ids_batch, then np.unique over each pattern's ids on the host;
    near_k1        search_near_ids_batch(patterns, 1): the floor (the same pieces and candidates, a cheaper compare, a
                   smaller answer);
    edit_k2        search_near_ids_batch(patterns, 2, edits=True), timed against
    near_k2        search_near_ids_batch(patterns, 2) alone: the enumeration within two edits is quadratic and is not run.
Before anything is timed edit_k1's answers are compared with variants_k1's pattern by pattern (sorted ids), and near_k's are
checked to lie inside edit_k's.  Each leg is warmed up, then timed `--reps` times with a host clock around the whole leg
(every library call ends in a stream synchronise); the legs alternate for `--rounds` rounds.  Reported: median / min / max
per leg and round, hits against entries and the device time (last_stats) of the leg's last search call.  No threshold: a
record, not a test."""
import json
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_patterns, time_legs, words_reader, write_json


def variants(word: bytes, alphabet: bytes):
    """The word and every string one edit away over the alphabet, each once."""
    out = {word}
    for i in range(len(word) + 1):
        out.update(word[:i] + bytes([x]) + word[i:] for x in alphabet)
        if i < len(word):
            out.add(word[:i] + word[i + 1:])
            out.update(word[:i] + bytes([x]) + word[i + 1:] for x in alphabet)
    return sorted(out)


def main():
    args = arguments('edit_vs_variants.json', ('--patterns', 32))
    r, text, alphabet = words_reader()
    patterns = pick_patterns(text.tobytes(), args.patterns)
    every = [variants(p, alphabet) for p in patterns]
    flat = [s for group in every for s in group]
    bounds_q = np.concatenate(([0], np.cumsum([len(g) for g in every])))
    seen = {}

    def near(k, edits):
        def leg():
            res = r.search_near_ids_batch(patterns, k, edits=edits)
            seen[f"{'edit' if edits else 'near'}_k{k}"] = r.last_stats()
            return per_row(res)
        return leg

    def variants_k1():
        res = r.search_ids_batch(flat)
        seen['variants_k1'] = r.last_stats()
        rows = per_row(res)
        return [np.unique(np.concatenate(rows[bounds_q[g]:bounds_q[g + 1]])) for g in range(len(patterns))]

    legs = {'edit_k1': near(1, True), 'variants_k1': variants_k1, 'near_k1': near(1, False), 'edit_k2': near(2, True), 'near_k2': near(2, False)}
    want = variants_k1()
    for g, (x, y) in enumerate(zip(legs['edit_k1'](), want)):
        if not np.array_equal(np.sort(x), y):
            raise SystemExit(f'edit_k1, pattern {g} {patterns[g]}: {x.size} ids against {y.size} of the variants')
    for k in (1, 2):
        for g, (x, y) in enumerate(zip(legs[f'edit_k{k}'](), legs[f'near_k{k}']())):
            if not np.isin(y, x).all():
                raise SystemExit(f'near_k{k}, pattern {g} {patterns[g]}: an id that edit_k{k} does not return')

    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds)
    r.close()
    summary = medians(runs, legs)
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_near_ids_batch(patterns, 1, edits=True) vs every string within one edit of every pattern over the bytes of the '
                   'corpus through search_ids_batch + np.unique per pattern (the route before), vs search_near_ids_batch(patterns, 1) (the '
                   'floor: Hamming, the same pieces), and the two at k = 2 against each other; same reader: one 64 MiB chunk of `words`; host '
                   'clock around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over '
                   'reps after warm-up; the legs alternate; the edit_k1 answers were compared with variants_k1 pattern by pattern before '
                   'the timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'patterns': [p.decode() for p in patterns],
           'alphabet_bytes': len(alphabet), 'variants_k1_total': len(flat),
           'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'median_ms_device': {name: round(statistics.median(x['ms_device_search_call'] for x in runs if x['leg'] == name), 4) for name in legs},
           'variants_k1_over_edit_k1': round(med['variants_k1'] / med['edit_k1'], 2),
           'edit_k1_over_near_k1': round(med['edit_k1'] / med['near_k1'], 2),
           'edit_k2_over_near_k2': round(med['edit_k2'] / med['near_k2'], 2)}
    write_json(out, args.out)
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'median_ms_device': out['median_ms_device'],
                      'variants_k1_over_edit_k1': out['variants_k1_over_edit_k1'], 'edit_k1_over_near_k1': out['edit_k1_over_near_k1'],
                      'edit_k2_over_near_k2': out['edit_k2_over_near_k2']}))


if __name__ == '__main__':
    main()
