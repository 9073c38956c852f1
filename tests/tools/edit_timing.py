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
    """The word and every string one edit away over the alphabet, each once."""
    out = {word}
    for i in range(len(word) + 1):
        out.update(word[:i] + bytes([x]) + word[i:] for x in alphabet)
        if i < len(word):
            out.add(word[:i] + word[i + 1:])
            out.update(word[:i] + bytes([x]) + word[i + 1:] for x in alphabet)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edit_vs_variants.json'))
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
    out = {'what': 'search_near_ids_batch(patterns, 1, edits=True) vs every string within one edit of every pattern over the bytes of the '
                   'corpus through search_ids_batch + np.unique per pattern (the route before), vs search_near_ids_batch(patterns, 1) (the '
                   'floor: Hamming, the same pieces), and the two at k = 2 against each other; same reader: one 64 MiB chunk of `words`; host '
                   'clock around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over '
                   'reps after warm-up; the legs alternate; the edit_k1 answers were compared with variants_k1 pattern by pattern before '
                   'the timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'patterns': [p.decode() for p in patterns],
           'alphabet_bytes': len(alphabet), 'variants_k1_total': len(flat),
           'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'median_ms_device': {name: round(statistics.median(x['ms_device_search_call'] for x in runs if x['leg'] == name), 4) for name in legs},
           'variants_k1_over_edit_k1': round(med['variants_k1'] / med['edit_k1'], 2),
           'edit_k1_over_near_k1': round(med['edit_k1'] / med['near_k1'], 2),
           'edit_k2_over_near_k2': round(med['edit_k2'] / med['near_k2'], 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'median_ms_device': out['median_ms_device'],
                      'variants_k1_over_edit_k1': out['variants_k1_over_edit_k1'], 'edit_k1_over_near_k1': out['edit_k1_over_near_k1'],
                      'edit_k2_over_near_k2': out['edit_k2_over_near_k2']}))


if __name__ == '__main__':
    main()
