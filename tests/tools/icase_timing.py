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
import argparse
import collections
import ctypes
import itertools
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


def pick_patterns(text: bytes, count: int):
    """`count` alphabetic words of 4 .. 10 letters, lower case, spread over the frequency ranking of the first 4 MiB."""
    words = collections.Counter(text[:4 << 20].lower().replace(b'\n', b' ').split(b' '))
    ranked = [w for w, _ in words.most_common() if 4 <= len(w) <= 10 and w.isalpha()]
    if len(ranked) < count:
        raise SystemExit(f'the corpus yields {len(ranked)} words of 4 .. 10 letters, {count} are wanted')
    span = min(len(ranked), 2000)
    return [ranked[i * span // count] for i in range(count)]


def spellings(word: bytes):
    return [bytes(c) for c in itertools.product(*[(b & ~0x20, b | 0x20) for b in word])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'icase_vs_variants.json'))
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
    mangle_words(text, np.random.default_rng(20))
    patterns = pick_patterns(text.tobytes(), args.patterns)
    every = [spellings(p) for p in patterns]
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

    legs = {f'icase_F{F}': (F, icase(F)) for F in (3, 4, 5, 6)}
    legs['all_spellings'] = (None, all_spellings)
    legs['plain'] = (None, plain)
    want = all_spellings()
    for name, (F, call) in legs.items():
        if F is None:
            continue
        set_letters(F)
        for g, (x, y) in enumerate(zip(call(), want)):
            if not np.array_equal(np.sort(x), y):
                raise SystemExit(f'{name}, pattern {g} {patterns[g]}: {x.size} ids against {y.size} of all spellings')

    runs = []
    for _ in range(args.rounds):
        for name, (F, call) in legs.items():
            set_letters(F)
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
    set_letters(None)
    r.close()
    summary = {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}
    med = {name: statistics.median(v) for name, v in summary.items()}
    out = {'what': 'search_icase_ids_batch(patterns) at PSS_ICASE_SEED_LETTERS = 3 .. 6 vs every spelling of every pattern through '
                   'search_ids_batch + np.unique per pattern (the route before), vs the lower-case patterns through search_ids_batch (the '
                   'floor), same reader: one 64 MiB chunk of `words`, about 1/8 of the words capitalised and 1/32 upper-cased; host clock '
                   'around the whole leg (packing the batch in Python and the host-side unique included), median / min / max over reps '
                   'after warm-up; the legs alternate; the icase answers were compared with all_spellings pattern by pattern before the '
                   'timing; hits / entries / ms_device are last_stats() of the leg\'s last search call',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'patterns': [p.decode() for p in patterns],
           'spellings_total': len(flat), 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'median_of_medians_ms': {k: round(v, 4) for k, v in med.items()},
           'all_spellings_over_icase_F5': round(med['all_spellings'] / med['icase_F5'], 2),
           'fastest_F': min((3, 4, 5, 6), key=lambda F: med[f'icase_F{F}'])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'median_of_medians_ms': out['median_of_medians_ms'], 'fastest_F': out['fastest_F']}))


if __name__ == '__main__':
    main()
