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
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CHUNK_BYTES = 64 << 20


def commit_hash():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'anchored_vs_plain.json'))
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    ap.add_argument('--queries', type=int, default=10000)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()

    import torch

    import pysubstringsearch_amd as P
    from pysubstringsearch_amd import _ffi
    if P.device_count() < 1:
        raise SystemExit('no HIP device: nothing to measure')

    n = CHUNK_BYTES
    text = np.empty(n, dtype=np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus(_ffi.CORPUS_LINES, text.ctypes.data, n, 0))
    sa = np.empty(n, dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(text.ctypes.data, sa.ctypes.data, n, 0))
    rng = np.random.default_rng(1)
    starts = np.flatnonzero(text[:-9] == 0x0A) + 1
    patterns = []
    while len(patterns) < args.queries:
        at_start = len(patterns) % 2 == 0
        s = int(starts[rng.integers(0, starts.size)]) if at_start else int(rng.integers(0, n - 8))
        q = text[s:s + 8].tobytes()
        if b'\n' not in q:
            patterns.append(q)

    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = P.Reader._from_handle(h)
    dt, ds = torch.from_numpy(text).cuda(), torch.from_numpy(sa).cuda()
    _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), n))
    del dt, ds

    legs = {'anchored_start': lambda: r.count_anchored_bytes(patterns, 'start'),
            'anchored_entry': lambda: r.count_anchored_bytes(patterns, 'entry'),
            'plain': lambda: r.count_multiple_bytes(patterns)}
    runs = []
    for _ in range(args.rounds):
        for name, call in legs.items():
            times = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                counts = call()
                t = time.perf_counter() - t0
                if i >= args.warmup:
                    times.append(t * 1e3)
            st = r.last_stats()
            runs.append({'leg': name, 'median_ms': round(statistics.median(times), 4), 'min_ms': round(min(times), 4),
                         'max_ms': round(max(times), 4), 'reps': args.reps, 'entries': int(sum(counts)),
                         'queries_with_entries': int(sum(1 for c in counts if c)), 'hits': int(st['hits']),
                         'ms_device_last_call': round(st['ms_device'], 4), 'ms_interval_last_call': round(st['ms_interval'], 4),
                         'route': hex(st['route'])})
    r.close()
    out = {'what': 'count_anchored_bytes (start, entry) vs count_multiple_bytes on one batch: one 64 MiB chunk of `lines`, patterns of 8 bytes cut '
                   'from the text (half at the start of an entry, half anywhere, no newline inside); host clock around the Python call (ends in a '
                   'stream synchronise inside the library, includes packing the batch in Python), median / min / max over reps after warm-up; '
                   'the three legs alternate',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'queries': len(patterns), 'warmup': args.warmup, 'reps': args.reps,
           'runs': runs,
           'summary': {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out['summary']))


if __name__ == '__main__':
    main()
