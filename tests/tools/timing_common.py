"""What the timing tools of this directory share (*_timing.py, ids_perf.py): the repository root and the commit, one chunk of
generated text on a device reader, patterns picked off its word-frequency ranking, the alternating timing loop with its
per-leg record, and the JSON writer.  Nothing of the library is imported until a function needs it: ids_perf.py measures
libraries it loads itself."""
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


def arguments(out_name, sized, warmup=3, reps=10):
    """The command line of a *_timing.py tool: --out (profiles/<out_name>), --commit, the tool's own size argument
    `sized` = (flag, default), --warmup, --reps, --rounds."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', out_name))
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    ap.add_argument(sized[0], type=int, default=sized[1])
    ap.add_argument('--warmup', type=int, default=warmup)
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--rounds', type=int, default=3)
    return ap.parse_args()


def words_reader(chunk_bytes=CHUNK_BYTES, corpus='words', close=True, edit=None):
    """(reader, text, alphabet): one chunk of pss_gen_corpus text -- closed with a newline unless close=False, changed in
    place by edit(text) if given --, its suffix array by pss_sa_build, handed to a reader on the device.  text is the
    numpy array, alphabet the bytes that occur in it without 0x0A."""
    import torch

    import pysubstringsearch_amd as P
    from pysubstringsearch_amd import _ffi
    if P.device_count() < 1:
        raise SystemExit('no HIP device: nothing to measure')
    n = chunk_bytes
    text = np.empty(n, dtype=np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus({'words': _ffi.CORPUS_WORDS, 'lines': _ffi.CORPUS_LINES}[corpus], text.ctypes.data, n, 0))
    if close:
        text[n - 1] = 0x0A
    if edit is not None:
        edit(text)
    alphabet = bytes(b for b in np.flatnonzero(np.bincount(text, minlength=256)).tolist() if b != 0x0A)
    sa = np.empty(n, dtype=np.int32)
    _ffi.check(_ffi.lib.pss_sa_build(text.ctypes.data, sa.ctypes.data, n, 0))
    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    r = P.Reader._from_handle(h)
    dt, ds = torch.from_numpy(text).cuda(), torch.from_numpy(sa).cuda()
    _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dt.data_ptr(), ds.data_ptr(), n))
    del dt, ds
    return r, text, alphabet


def pick_patterns(text: bytes, count: int, lo: int = 8, hi: int = 12, fold: bool = False):
    """`count` alphabetic words of lo .. hi letters (lower-cased first if fold), spread over the frequency ranking of the
    first 4 MiB."""
    head = text[:4 << 20].lower() if fold else text[:4 << 20]
    words = collections.Counter(head.replace(b'\n', b' ').split(b' '))
    ranked = [w for w, _ in words.most_common() if lo <= len(w) <= hi and w.isalpha()]
    if len(ranked) < count:
        raise SystemExit(f'the corpus yields {len(ranked)} words of {lo} .. {hi} letters, {count} are wanted')
    span = min(len(ranked), 2000)
    return [ranked[i * span // count] for i in range(count)]


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


def per_row(res):
    """The ids of an IdResult, one array per row of the batch."""
    b = np.concatenate(([0], np.cumsum(res.counts.astype(np.int64))))
    return [res.ids[b[g]:b[g + 1]] for g in range(len(res.counts))]


def spread(times, reps):
    return {'median_ms': round(statistics.median(times), 4), 'min_ms': round(min(times), 4), 'max_ms': round(max(times), 4), 'reps': reps}


def search_call_record(out, st):
    """What a leg found and the statistics of its search call, under the names most of the tools write."""
    return {'entries': int(sum(x.size for x in out)), 'queries_search_call': int(st['queries']), 'hits_search_call': int(st['hits']),
            'entries_search_call': int(st['entries']), 'ms_device_search_call': round(st['ms_device'], 4),
            'ms_interval_search_call': round(st['ms_interval'], 4), 'route': hex(st['route'])}


def time_legs(legs, seen, warmup, reps, rounds, record=search_call_record, before=None):
    """Every leg of legs = {name: call} warmed up `warmup` times and timed `reps` times with a host clock around the call,
    the legs alternating for `rounds` rounds.  One record per leg and round: median / min / max, then
    record(the call's last return value, seen(name)), seen(name) being the statistics the record is to show -- a dict the
    legs fill, or a function.  before(name), if given, runs ahead of a leg's calls, untimed.  Where those statistics carry
    ms_host (the library's own host clock around its last search call), its median / min / max over the timed calls are
    recorded too: what a change to the host driver alone can move."""
    runs = []
    for _ in range(rounds):
        for name, call in legs.items():
            if before is not None:
                before(name)
            times, host = [], []
            for i in range(warmup + reps):
                t0 = time.perf_counter()
                out = call()
                t = time.perf_counter() - t0
                if i >= warmup:
                    times.append(t * 1e3)
                    st = seen(name) if callable(seen) else seen.get(name)
                    if st is not None and 'ms_host' in st:
                        host.append(st['ms_host'])
            st = seen(name) if callable(seen) else seen[name]
            runs.append({'leg': name, **spread(times, reps), **record(out, st)})
            if host:
                runs[-1]['ms_host_last_call'] = {k: v for k, v in spread(host, reps).items() if k != 'reps'}
    return runs


def medians(runs, legs):
    """{leg: its median of every round}."""
    return {name: [x['median_ms'] for x in runs if x['leg'] == name] for name in legs}


def write_json(out, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
