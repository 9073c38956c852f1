"""Anchored counts next to the plain count on the same batch (MI355X; run by hand, not by the suite):

    python tests/tools/anchored_timing.py [--commit HASH] [--out profiles/anchored_vs_plain.json]

One 64 MiB chunk of `lines` text (pss_gen_corpus), its suffix array by pss_sa_build, handed to a reader on the device.
The batch: 10 000 patterns of 8 bytes cut from the text, none with a newline inside -- half of them at the start of an
entry (so that 'start' has something to find), half anywhere.  Three legs on that batch:
    count_anchored_bytes(patterns, 'start'), count_anchored_bytes(patterns, 'entry'), count_multiple_bytes(patterns).
Each leg is warmed up, then timed `--reps` times with a host clock around the call (every call ends in a stream
synchronise inside the library); the legs alternate for `--rounds` rounds, so the spread between two runs of the same
leg is on record next to the differences between the legs.  Reported: median / min / max per leg and round, the
library's own device time of the last call (last_stats), and what each leg found.  No threshold: a record, not a test."""
import json

import numpy as np

from timing_common import arguments, commit_hash, medians, time_legs, words_reader, write_json


def main():
    args = arguments('anchored_vs_plain.json', ('--queries', 10000), warmup=5, reps=50)
    r, text, _ = words_reader(corpus='lines', close=False)
    n = text.size
    rng = np.random.default_rng(1)
    starts = np.flatnonzero(text[:-9] == 0x0A) + 1
    patterns = []
    while len(patterns) < args.queries:
        at_start = len(patterns) % 2 == 0
        s = int(starts[rng.integers(0, starts.size)]) if at_start else int(rng.integers(0, n - 8))
        q = text[s:s + 8].tobytes()
        if b'\n' not in q:
            patterns.append(q)

    legs = {'anchored_start': lambda: r.count_anchored_bytes(patterns, 'start'),
            'anchored_entry': lambda: r.count_anchored_bytes(patterns, 'entry'),
            'plain': lambda: r.count_multiple_bytes(patterns)}

    def record(counts, st):
        return {'entries': int(sum(counts)), 'queries_with_entries': int(sum(1 for c in counts if c)), 'hits': int(st['hits']),
                'ms_device_last_call': round(st['ms_device'], 4), 'ms_interval_last_call': round(st['ms_interval'], 4),
                'route': hex(st['route'])}

    runs = time_legs(legs, lambda name: r.last_stats(), args.warmup, args.reps, args.rounds, record)
    r.close()
    out = {'what': 'count_anchored_bytes (start, entry) vs count_multiple_bytes on one batch: one 64 MiB chunk of `lines`, patterns of 8 bytes cut '
                   'from the text (half at the start of an entry, half anywhere, no newline inside); host clock around the Python call (ends in a '
                   'stream synchronise inside the library, includes packing the batch in Python), median / min / max over reps after warm-up; '
                   'the three legs alternate',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'queries': len(patterns), 'warmup': args.warmup, 'reps': args.reps,
           'runs': runs,
           'summary': medians(runs, legs)}
    write_json(out, args.out)
    print(json.dumps(out['summary']))


if __name__ == '__main__':
    main()
