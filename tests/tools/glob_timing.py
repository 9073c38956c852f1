"""The wildcard search next to the route that existed before it, on the same patterns (MI355X; run by hand, not by the suite):

    python tests/tools/glob_timing.py [--commit HASH] [--out profiles/glob_vs_host_filter.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  The patterns pair a FREQUENT word with a RARE one, in both orders: `*FREQUENT*RARE*` and
`*RARE*FREQUENT*` for each of `--pairs` pairs (the words are picked as tests/tools/all_terms_timing.py picks them).  Two
legs on those patterns, on the same reader:
    glob          search_glob_ids_batch(patterns): one device call, the rarest segment drives, the order is verified on
                  the device;
    host_filter   search_all_ids_batch([[f, x]] per pattern), entries_by_id_packed(ids), a Python `re` over every
                  candidate's text on the host, then indexing the ids: every candidate's text crosses PCIe.
Before anything is timed the two legs' answers are compared pattern by pattern (sorted ids).  Each leg is warmed up, then
timed `--reps` times with a host clock around the whole leg (every library call ends in a stream synchronise); the legs
alternate for `--rounds` rounds, so the spread between two runs of the same leg is on record next to the difference
between the legs.  Reported: median / min / max per leg and round, hits and device time (last_stats) of the leg's search
call, and the ratio of the medians.  No threshold: a record, not a test.  With rare words for drivers the candidates are
few, so this says what the two extra trips cost on a small answer -- and nothing about the verify kernel's shape: 8 lanes
against one lane per candidate stays unmeasured."""
import argparse
import collections
import re
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'glob_vs_host_filter.json'))
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
    text[n - 1] = 0x0A              # (every entry closed: the text handed out by id is then every entry's whole text)
    frequent, rare = pick_terms(text.tobytes(), args.pairs)
    segs = []
    for f, x in zip(frequent, rare):
        segs += [(f, x), (x, f)]
    patterns = [b'*' + P.glob_escape(a) + b'*' + P.glob_escape(b) + b'*' for a, b in segs]
    groups = [[a, b] for a, b in segs]
    filters = [re.compile(b'.*' + re.escape(a) + b'.*' + re.escape(b) + b'.*', re.DOTALL) for a, b in segs]
    sa = np.empty(n, dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(text.ctypes.data, sa.ctypes.data, n, 0))

    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = P.Reader._from_handle(h)
    dt, ds = torch.from_numpy(text).cuda(), torch.from_numpy(sa).cuda()
    _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), n))
    del dt, ds
    seen = {}

    def glob():
        res = r.search_glob_ids_batch(patterns)
        seen['glob'] = r.last_stats()
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64))))
        return [res.ids[bounds[g]:bounds[g + 1]] for g in range(len(patterns))]

    def host_filter():
        res = r.search_all_ids_batch(groups)
        seen['host_filter'] = r.last_stats()
        pk = r.entries_by_id_packed(res.ids)
        data, o = pk.data.tobytes(), pk.offsets.tolist()
        bounds = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64)))).tolist()
        out = []
        for g, rx in enumerate(filters):
            keep = [i for i in range(bounds[g], bounds[g + 1]) if rx.fullmatch(data, o[i], o[i + 1])]
            out.append(res.ids[keep])
        return out

    a, b = glob(), host_filter()
    for g, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(np.sort(x), np.sort(y)):
            raise SystemExit(f'pattern {g} {patterns[g]}: the two legs disagree ({x.size} against {y.size} ids)')
    candidates = int(r.search_all_ids_batch(groups).ids.size)

    legs = {'glob': glob, 'host_filter': host_filter}
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
                         'hits_search_call': int(st['hits']), 'entries_search_call': int(st['entries']),
                         'ms_device_search_call': round(st['ms_device'], 4), 'ms_interval_search_call': round(st['ms_interval'], 4),
                         'route': hex(st['route'])})
    r.close()
    summary = {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}
    ratio = statistics.median(summary['host_filter']) / statistics.median(summary['glob'])
    out = {'what': 'search_glob_ids_batch(patterns) vs search_all_ids_batch + entries_by_id_packed + a host `re` over every candidate + '
                   'indexing the ids, same reader: one 64 MiB chunk of `words`, patterns *FREQUENT*RARE* and *RARE*FREQUENT*; host clock '
                   'around the whole leg (every library call ends in a stream synchronise; packing the batch in Python and the host filter '
                   'included), median / min / max over reps after warm-up; the two legs alternate; the answers were compared pattern by '
                   'pattern before the timing; ms_device is last_stats() of the leg\'s search call (the glob call, the all-terms call)',
           'commit': args.commit or commit_hash(), 'chunk_bytes': n, 'patterns': len(patterns), 'candidates_all_terms': candidates,
           'entries_glob': int(sum(x.size for x in a)), 'warmup': args.warmup, 'reps': args.reps, 'runs': runs, 'summary': summary,
           'host_filter_over_glob': round(ratio, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'summary': summary, 'host_filter_over_glob': out['host_filter_over_glob']}))


if __name__ == '__main__':
    main()
