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


def pick_patterns(text: bytes, count: int):
    """`count` alphabetic words of 8 .. 12 letters, spread over the frequency ranking of the first 4 MiB."""
    words = collections.Counter(text[:4 << 20].replace(b'\n', b' ').split(b' '))
    ranked = [w for w, _ in words.most_common() if 8 <= len(w) <= 12 and w.isalpha()]
    if len(ranked) < count:
        raise SystemExit(f'the corpus yields {len(ranked)} words of 8 .. 12 letters, {count} are wanted')
    span = min(len(ranked), 2000)
    return [ranked[i * span // count] for i in range(count)]


def variants(word: bytes, alphabet: bytes):
    """The word and every word one substitution away over the alphabet."""
    out = [word]
    for i, b in enumerate(word):
        out += [word[:i] + bytes([x]) + word[i + 1:] for x in alphabet if x != b]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'near_vs_variants.json'))
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    ap.add_argument('--patterns', type=int, default=32)
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
    text[n - 1] = 0x0A
    alphabet = bytes(b for b in np.flatnonzero(np.bincount(text, minlength=256)).tolist() if b != 0x0A)
    patterns = pick_patterns(text.tobytes(), args.patterns)
    every = [variants(p, alphabet) for p in patterns]
    flat = [s for group in every for s in group]
    bounds_q = np.concatenate(([0], np.cumsum([len(g) for g in every])))
    a1 = len(alphabet) - 1
    variants_k2 = sum(1 + len(p) * a1 + len(p) * (len(p) - 1) // 2 * a1 * a1 for p in patterns)
    sa = np.empty(n, dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(text.ctypes.data, sa.ctypes.data, n, 0))

    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = P.Reader._from_handle(h)
    dt, ds = torch.from_numpy(text).cuda(), torch.from_numpy(sa).cuda()
    _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), n))
    del dt, ds
    seen = {}

    def per_row(res):
        b = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64))))
        return [res.ids[b[g]:b[g + 1]] for g in range(len(res.counts))]

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
            st = seen[name]
            runs.append({'leg': name, 'median_ms': round(statistics.median(times), 4), 'min_ms': round(min(times), 4),
                         'max_ms': round(max(times), 4), 'reps': args.reps, 'entries': int(sum(x.size for x in out)),
                         'queries_search_call': int(st['queries']), 'hits_search_call': int(st['hits']),
                         'entries_search_call': int(st['entries']), 'ms_device_search_call': round(st['ms_device'], 4),
                         'ms_interval_search_call': round(st['ms_interval'], 4), 'route': hex(st['route'])})
    r.close()
    summary = {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_near_ids_batch(patterns, 1) vs every one-substitution variant of every pattern over the bytes of the corpus '
                   'through search_ids_batch + np.unique per pattern (the route before), vs the patterns through search_ids_batch (the '
                   'floor), and search_near_ids_batch(patterns, 2) against itself; same reader: one 64 MiB chunk of `words`; host clock '
                   'around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over reps '
                   'after warm-up; the legs alternate; the near_k1 answers were compared with variants_k1 pattern by pattern before the '
                   'timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'patterns': [p.decode() for p in patterns],
           'alphabet_bytes': len(alphabet), 'variants_k1_total': len(flat), 'variants_k2_total_not_run': variants_k2,
           'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'variants_k1_over_near_k1': round(med['variants_k1'] / med['near_k1'], 2),
           'near_k1_over_plain': round(med['near_k1'] / med['plain'], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'variants_k1_over_near_k1': out['variants_k1_over_near_k1']}))


if __name__ == '__main__':
    main()
