"""The all-terms search next to ids + numpy set operations on the same groups (MI355X; run by hand, not by the suite):

    python tests/tools/all_terms_timing.py [--commit HASH] [--out profiles/all_terms_vs_ids.json]

One 64 MiB chunk of `words` text (pss_gen_corpus), its suffix array by pss_sa_build, handed to a reader on the device.
The groups pair a FREQUENT term with a RARE one, in both orders: the `--pairs` most frequent words of a sample of the text
(each in a large share of the entries) against as many words that occur a handful of times, [frequent, rare] and
[rare, frequent] for every pair.  Two legs on those groups, on the same reader:
    all_terms   search_all_ids_batch(groups): one device call, the rarest term of every group drives;
    ids_numpy   search_ids_batch(distinct terms), then np.intersect1d per group on the host: what the README recommended
                before the device call existed.  Every id of every term comes through the pipeline and over PCIe.
Before anything is timed the two legs' answers are compared group by group (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg (every library call ends in a stream synchronise); the legs
alternate for `--rounds` rounds, so the spread between two runs of the same leg is on record next to the difference
between the legs.  Reported: median / min / max per leg and round, hits and device time of the leg's last library
call (last_stats), and the ratio of the medians.  No threshold: a record, not a test."""
import argparse
import collections
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


def pick_terms(text: bytes, pairs: int):
    """(frequent, rare): the most frequent words of the first 4 MiB, and words of >= 6 bytes that occur 1 .. 40 times in the
    whole text."""
    words = collections.Counter(text[:4 << 20].replace(b'\n', b' ').split(b' '))
    words.pop(b'', None)
    ranked = [w for w, _ in words.most_common()]
    frequent = ranked[:pairs]
    rare = []
    for w in reversed(ranked):
        if len(w) >= 6 and w not in frequent and 1 <= text.count(w) <= 40:
            rare.append(w)
            if len(rare) == pairs:
                break
    if len(frequent) < pairs or len(rare) < pairs:
        raise SystemExit(f'the corpus yields {len(frequent)} frequent and {len(rare)} rare words, {pairs} of each are wanted')
    return frequent, rare


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'all_terms_vs_ids.json'))
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()

    import torch

    import pysubstringsearch_amd as P
    from pysubstringsearch_amd import _ffi
    if P.device_count() < 1:
        raise SystemExit('no HIP device: nothing to measure')

    n = CHUNK_BYTES
    text = np.empty(n, dtype=np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus(_ffi.CORPUS_WORDS, text.ctypes.data, n, 0))
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    groups = []
    for f, x in zip(frequent, rare):
        groups += [[f, x], [x, f]]
    terms = sorted(set(frequent + rare))
    term_at = {t: i for i, t in enumerate(terms)}
    sa = np.empty(n, dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(text.ctypes.data, sa.ctypes.data, n, 0))

    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = P.Reader._from_handle(h)
    dt, ds = torch.from_numpy(text).cuda(), torch.from_numpy(sa).cuda()
    _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), n))
    del dt, ds

    def all_terms():
        res = r.search_all_ids_batch(groups)
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64))))
        return [res.ids[bounds[g]:bounds[g + 1]] for g in range(len(groups))]

    def ids_numpy():
        res = r.search_ids_batch(terms)
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64))))
        per = [res.ids[bounds[t]:bounds[t + 1]] for t in range(len(terms))]
        return [np.intersect1d(per[term_at[a]], per[term_at[b]], assume_unique=True) for a, b in groups]

    a, b = all_terms(), ids_numpy()
    for g, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(np.sort(x), y):
            raise SystemExit(f'group {g} {groups[g]}: the two legs disagree ({x.size} against {y.size} ids)')
    term_entries = {t.decode('latin-1'): int(c) for t, c in zip(terms, r.search_ids_batch(terms).counts)}

    legs = {'all_terms': all_terms, 'ids_numpy': ids_numpy}
    runs = []
    for _ in range(args.rounds):
        for name, call in legs.items():
            times = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                out = call()
                t = time.perf_counter() - t0
                if i >= args.warmup:
                    times.append(t * 1e3)
            st = r.last_stats()
            runs.append({'leg': name, 'median_ms': round(statistics.median(times), 4), 'min_ms': round(min(times), 4),
                         'max_ms': round(max(times), 4), 'reps': args.reps, 'entries': int(sum(x.size for x in out)),
                         'hits_last_call': int(st['hits']), 'entries_last_call': int(st['entries']),
                         'result_bytes_last_call': int(st['result_bytes']), 'ms_device_last_call': round(st['ms_device'], 4),
                         'ms_interval_last_call': round(st['ms_interval'], 4), 'route': hex(st['route'])})
    r.close()
    summary = {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}
    ratio = statistics.median(summary['ids_numpy']) / statistics.median(summary['all_terms'])
    out = {'what': 'search_all_ids_batch(groups) vs search_ids_batch(distinct terms) + np.intersect1d per group, same reader: one 64 MiB chunk '
                   'of `words`, groups [frequent word, rare word] and [rare, frequent]; host clock around the whole leg (every library call '
                   'ends in a stream synchronise; packing the batch in Python and the numpy set operations included), median / min / max '
                   'over reps after warm-up; the two legs alternate; the answers were compared group by group before the timing',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'groups': len(groups), 'distinct_terms': len(terms),
           'entries_per_term': term_entries, 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'ids_numpy_over_all_terms': round(ratio, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'summary': summary, 'ids_numpy_over_all_terms': out['ids_numpy_over_all_terms']}))


if __name__ == '__main__':
    main()
