"""The case-insensitive search next to the route that existed before it, on the same patterns (MI355X; run by hand, not by the
suite):

    python tests/tools/icase_timing.py [--commit HASH] [--out profiles/icase_vs_variants.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline) whose words are case-mangled with numpy -- about
1/8 of them capitalised, about 1/32 upper-cased --, its suffix array by pss_sa_build, handed to a reader on the device.  32
patterns of 4 .. 10 letters, words of the text spread over its frequency ranking.  The legs, on the same reader:
    icase_F3 .. icase_F6   search_icase_ids_batch(patterns) with PSS_ICASE_SEED_LETTERS = 3, 4, 5, 6: one device call;
    all_spellings          the route the engine had before: every one of the 2^L spellings of every pattern through
                           search_ids_batch, then np.unique over each pattern's ids on the host;
    plain                  the same patterns, lower case, through search_ids_batch: the floor (it answers another question).
Before anything is timed the icase legs' answers are compared with all_spellings' pattern by pattern (sorted ids).  Each leg
is warmed up, then timed `--reps` times with a host clock around the whole leg (every library call ends in a stream
synchronise); the legs alternate for `--rounds` rounds.  Reported: median / min / max per leg and round, hits against
entries and the device time (last_stats) of the leg's last search call.  No threshold: a record, not a test."""
import itertools
import json
import os
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, per_row, pick_patterns, time_legs, words_reader, write_json


def mangle_words(text: np.ndarray, rng) -> None:
    """In place: about 1/8 of the words capitalised, about 1/32 upper-cased."""
    lower = (text >= 0x61) & (text <= 0x7A)
    sep = (text == 0x20) | (text == 0x0A)
    start = np.empty(text.size, dtype=bool)
    start[0] = True
    start[1:] = sep[:-1]
    word = np.cumsum(start, dtype=np.int32) - 1
    u = rng.random(int(word[-1]) + 1, dtype=np.float32)
    cap, upper = u < 1 / 8, (u >= 1 / 8) & (u < 1 / 8 + 1 / 32)
    text[(start & lower & cap[word]) | (lower & upper[word])] ^= 0x20


def spellings(word: bytes):
    return [bytes(c) for c in itertools.product(*[(b & ~0x20, b | 0x20) for b in word])]


def main():
    args = arguments('icase_vs_variants.json', ('--patterns', 32))
    r, text, _ = words_reader(edit=lambda t: mangle_words(t, np.random.default_rng(20)))
    from pysubstringsearch_amd import _ffi
    patterns = pick_patterns(text.tobytes(), args.patterns, 4, 10, fold=True)
    every = [spellings(p) for p in patterns]
    flat = [s for group in every for s in group]
    bounds_q = np.concatenate(([0], np.cumsum([len(g) for g in every])))
    seen = {}

    def icase(F):
        def leg():
            res = r.search_icase_ids_batch(patterns)
            seen[f'icase_F{F}'] = r.last_stats()
            return per_row(res)
        return leg

    def all_spellings():
        res = r.search_ids_batch(flat)
        seen['all_spellings'] = r.last_stats()
        rows = per_row(res)
        return [np.unique(np.concatenate(rows[bounds_q[g]:bounds_q[g + 1]])) for g in range(len(patterns))]

    def plain():
        res = r.search_ids_batch(patterns)
        seen['plain'] = r.last_stats()
        return per_row(res)

    def set_letters(F):
        if F is None:
            os.environ.pop('PSS_ICASE_SEED_LETTERS', None)
        else:
            os.environ['PSS_ICASE_SEED_LETTERS'] = str(F)
        _ffi.check(_ffi.lib.pss_reload_env())

    letters = {f'icase_F{F}': F for F in (3, 4, 5, 6)}
    legs = {name: icase(F) for name, F in letters.items()}
    legs['all_spellings'] = all_spellings
    legs['plain'] = plain
    want = all_spellings()
    for name, F in letters.items():
        set_letters(F)
        for g, (x, y) in enumerate(zip(legs[name](), want)):
            if not np.array_equal(np.sort(x), y):
                raise SystemExit(f'{name}, pattern {g} {patterns[g]}: {x.size} ids against {y.size} of all spellings')

    runs = time_legs(legs, seen, args.warmup, args.reps, args.rounds, before=lambda name: set_letters(letters.get(name)))
    set_letters(None)
    r.close()
    summary = medians(runs, legs)
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_icase_ids_batch(patterns) at PSS_ICASE_SEED_LETTERS = 3 .. 6 vs every spelling of every pattern through '
                   'search_ids_batch + np.unique per pattern (the route before), vs the lower-case patterns through search_ids_batch (the '
                   'floor), same reader: one 64 MiB chunk of `words`, about 1/8 of the words capitalised and 1/32 upper-cased; host clock '
                   'around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over reps '
                   'after warm-up; the legs alternate; the icase answers were compared with all_spellings pattern by pattern before the '
                   'timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': text.size, 'patterns': [p.decode() for p in patterns],
           'spellings_total': len(flat), 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'all_spellings_over_icase_F5': round(med['all_spellings'] / med['icase_F5'], 2),
           'fastest_F': min((3, 4, 5, 6), key=lambda F: med[f'icase_F{F}'])}
    write_json(out, args.out)
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'fastest_F': out['fastest_F']}))


if __name__ == '__main__':
    main()
