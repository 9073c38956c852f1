"""The search within k mismatches / k edits under ASCII case folding next to the route that existed before it, on the same
patterns (MI355X; run by hand, not by the suite):

    python tests/tools/near_icase_timing.py [--commit HASH] [--out profiles/near_icase_vs_variants.json]

The case-mangled 64 MiB `words` chunk of icase_timing.py (about 1/8 of the words capitalised, about 1/32 upper-cased), its
suffix array by pss_sa_build, handed to a reader on the device.  Near's 32 patterns: words of 8 .. 12 letters spread over the
frequency ranking of the folded text.  The legs, on the same reader:
    near_icase_k1 / edit_icase_k1   search_near_ids_batch(patterns, 1, icase=True) without and with edits=True: one device call;
    near_variants_k1                the route the engine had before: every string within one SUBSTITUTION of every pattern over
                                    the folded bytes of the corpus (near_timing.variants), through search_icase_ids_batch, then
                                    np.unique over each pattern's ids on the host;
    edit_variants_k1                the same with every string within one EDIT (edit_timing.variants);
    near_icase_k2 / edit_icase_k2   k = 2, timed against the floors only (their enumerations are quadratic and were not run);
    near_k1, edit_k1, near_k2, edit_k2   the floor of each: search_near_ids_batch(patterns, k, edits=...) in exact bytes;
    icase                           the other floor: search_icase_ids_batch(patterns).  (Both floors answer another question.)
Before anything is timed the answers of near_icase_k1 and edit_icase_k1 are compared with their variants' pattern by pattern
(sorted ids), and every fold answer must contain its exact-byte floor's.  Each leg is warmed up, then timed `--reps` times with
a host clock around the whole leg (every library call ends in a stream synchronise); the legs alternate for `--rounds` rounds.
Reported: median / min / max per leg and round, hits against entries and the device time (last_stats) of the leg's last search
call.  No threshold: a record, not a test."""
import json
import statistics

import numpy as np

from edit_timing import variants as edit_variants
from icase_timing import mangle_words
from near_timing import variants as near_variants
from timing_common import arguments, commit_hash, medians, per_row, pick_patterns, time_legs, words_reader, write_json


def main():
    args = arguments('near_icase_vs_variants.json', ('--patterns', 32))
    r, text, alphabet = words_reader(edit=lambda t: mangle_words(t, np.random.default_rng(20)))
    patterns = pick_patterns(text.tobytes(), args.patterns, fold=True)
    folded = bytes(sorted(set(alphabet.lower())))
    seen = {}

    def near(k, edits, icase):
        name = f"{'edit' if edits else 'near'}{'_icase' if icase else ''}_k{k}"

        def leg():
            res = r.search_near_ids_batch(patterns, k, edits=edits, icase=icase)
            seen[name] = r.last_stats()
            return per_row(res)
        return name, leg

    def through_icase(name, every):
        flat = [s for group in every for s in group]
        bounds_q = np.concatenate(([0], np.cumsum([len(g) for g in every])))

        def leg():
            res = r.search_icase_ids_batch(flat)
            seen[name] = r.last_stats()
            rows = per_row(res)
            return [np.unique(np.concatenate(rows[bounds_q[g]:bounds_q[g + 1]])) for g in range(len(patterns))]
        return len(flat), leg

    def icase():
        res = r.search_icase_ids_batch(patterns)
        seen['icase'] = r.last_stats()
        return per_row(res)

    n_near, near_var = through_icase('near_variants_k1', [near_variants(p, folded) for p in patterns])
    n_edit, edit_var = through_icase('edit_variants_k1', [edit_variants(p, folded) for p in patterns])
    legs = dict([near(1, False, True), ('near_variants_k1', near_var), near(1, True, True), ('edit_variants_k1', edit_var),
                 near(2, False, True), near(2, True, True), near(1, False, False), near(1, True, False), near(2, False, False),
                 near(2, True, False), ('icase', icase)])
    for fold, var in (('near_icase_k1', 'near_variants_k1'), ('edit_icase_k1', 'edit_variants_k1')):
        for g, (x, y) in enumerate(zip(legs[fold](), legs[var]())):
            if not np.array_equal(np.sort(x), y):
                raise SystemExit(f'{fold}, pattern {g} {patterns[g]}: {x.size} ids against {y.size} of the variants')
    more = {}
    for kind in ('near', 'edit'):
        for k in (1, 2):
            rows = list(zip(legs[f'{kind}_icase_k{k}'](), legs[f'{kind}_k{k}']()))
            if any(np.setdiff1d(y, x).size for x, y in rows):
                raise SystemExit(f'{kind}_icase_k{k} does not contain {kind}_k{k}')
            more[f'{kind}_k{k}'] = [int(sum(x.size for x, _ in rows)), int(sum(y.size for _, y in rows))]

    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds)
    r.close()
    summary = medians(runs, legs)
    med = {name: statistics.median(v) for name, v in summary.items()}
    device = {name: round(statistics.median(x['ms_device_search_call'] for x in runs if x['leg'] == name), 4) for name in legs}
    out = {'what': 'search_near_ids_batch(patterns, k, icase=True), without and with edits=True, at k = 1 vs every string within one '
                   'substitution / one edit of every pattern over the folded bytes of the corpus through search_icase_ids_batch + np.unique '
                   'per pattern (the route before), and at k = 1, 2 vs two floors on the same reader: the exact-byte search_near_ids_batch at '
                   'the same k and search_icase_ids_batch of the patterns; one 64 MiB chunk of `words`, about 1/8 of the words capitalised '
                   'and 1/32 upper-cased; host clock around the whole leg (packing the batch in Python and the host-side unique included), '
                   'median / min / max over reps after warm-up; the legs alternate; the k = 1 answers were compared with the variants\' '
                   'pattern by pattern before the timing and every fold answer contains its exact-byte floor\'s; hits / entries / ms_device '
                   'are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'patterns': [p.decode() for p in patterns],
           'folded_alphabet_bytes': len(folded), 'near_variants_k1_total': n_near, 'edit_variants_k1_total': n_edit,
           'entries_fold_vs_exact': more, 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()}, 'median_ms_device': device,
           'near_variants_k1_over_near_icase_k1': round(med['near_variants_k1'] / med['near_icase_k1'], 2),
           'edit_variants_k1_over_edit_icase_k1': round(med['edit_variants_k1'] / med['edit_icase_k1'], 2),
           'over_exact_floor': {f'{kind}_k{k}': round(med[f'{kind}_icase_k{k}'] / med[f'{kind}_k{k}'], 2) for kind in ('near', 'edit') for k in (1, 2)},
           'over_icase_floor': {f'{kind}_k{k}': round(med[f'{kind}_icase_k{k}'] / med['icase'], 2) for kind in ('near', 'edit') for k in (1, 2)}}
    write_json(out, args.out)
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'median_ms_device': device}))


if __name__ == '__main__':
    main()
