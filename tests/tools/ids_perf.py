"""Entry ids against the packed search on the same hit-heavy batch (MI355X): what does asking WHICH entries match cost
next to fetching their text?

    python tests/tools/ids_perf.py [--parent-lib PATH/libpss.so] [--out profiles/entry_ids_vs_packed.json]

The index: 15 chunks of 1 MiB of `words` text (pss_gen_corpus), suffix arrays by pss_sa_build, written as a reference
container and opened with pss_reader_open.  The batch: queries of 4 .. 8 bytes cut from the text.  Every leg runs in a
fresh child process that talks to the library through plain ctypes (so the same code times a library built from the
parent commit, which lacks the new entry points: --parent-lib), warms up, then times `--reps` calls with a host clock
around the call (each call ends in a stream synchronise inside the library) and reports median, min and max.  The legs
alternate (parent, this, parent, this, ...) so that the spread between two runs of the SAME library is on record next
to the difference between the two.  The time to build the line tables (the first pss_reader_chunk_entries call of a
fresh reader) and the ids batch are measured for every block size PSS_LINE_BLOCK_SHIFT allows."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

from timing_common import ROOT, spread, write_json

CHUNKS, CHUNK_BYTES, CORPUS_WORDS = 15, 1 << 20, 1


def load(path):
    sys.path.insert(0, ROOT)
    try:        # one HIP runtime per process: the copy torch bundles, when torch is installed (as _ffi.py does)
        import importlib.util
        spec = importlib.util.find_spec('torch')
        cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so') if spec else ''
        if cand and os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except (ImportError, ValueError, OSError):
        pass
    L = ctypes.CDLL(path)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    pvp = ctypes.POINTER(vp)
    sig = {'pss_gen_corpus': (ctypes.c_int, [ctypes.c_int, vp, u64, u64]), 'pss_sa_build': (i32, [vp, vp, i32, i32]),
           'pss_reader_open': (ctypes.c_int, [ctypes.c_char_p, i32, i32, i32, pvp]), 'pss_reader_close': (ctypes.c_int, [vp]),
           'pss_reader_search_batch': (ctypes.c_int, [vp, vp, vp, u32, pvp]), 'pss_result_num_entries': (u64, [vp]),
           'pss_result_offsets': (ctypes.POINTER(u64), [vp]), 'pss_result_free': (None, [vp]),
           'pss_reader_residency': (ctypes.c_int, [vp, ctypes.POINTER(u64), vp, vp]),
           'pss_last_error': (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t])}
    if hasattr(L, 'pss_reader_search_ids_batch'):
        sig['pss_reader_search_ids_batch'] = (ctypes.c_int, [vp, vp, vp, u32, pvp])
        sig['pss_reader_chunk_entries'] = (ctypes.c_int, [vp, vp, vp, u64, ctypes.POINTER(u64)])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def ok(L, rc):
    if rc != 0:
        buf = ctypes.create_string_buffer(1024)
        L.pss_last_error(buf, len(buf))
        raise RuntimeError(f'libpss error {rc}: {buf.value.decode("utf-8", "replace")}')


def write_index(L, path, nq, seed=1):
    """The index file and the query batch (blob, u64 offsets)."""
    rng = np.random.default_rng(seed)
    queries = []
    with open(path, 'wb') as f:
        for c in range(CHUNKS):
            text = np.empty(CHUNK_BYTES, dtype=np.uint8)
            ok(L, L.pss_gen_corpus(CORPUS_WORDS, text.ctypes.data, CHUNK_BYTES, c))
            sa = np.empty(CHUNK_BYTES, dtype=np.int32)
            ok(L, L.pss_sa_build(text.ctypes.data, sa.ctypes.data, CHUNK_BYTES, 0))
            f.write(np.uint32(CHUNK_BYTES).tobytes() + text.tobytes() + np.uint32(4 * CHUNK_BYTES).tobytes() + sa.astype('<i4').tobytes())
            while len(queries) < (c + 1) * nq // CHUNKS:
                s, ln = int(rng.integers(0, CHUNK_BYTES - 8)), int(rng.integers(4, 9))
                q = text[s:s + ln].tobytes()
                if b'\n' not in q:
                    queries.append(q)
    offs = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum([len(q) for q in queries], out=offs[1:])
    return b''.join(queries), offs


def timed(L, call, h, blob, offs, warmup, reps):
    nq = len(offs) - 1
    times, entries, nbytes = [], 0, 0
    for i in range(warmup + reps):
        res = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = call(h, blob, offs.ctypes.data, nq, ctypes.byref(res))
        dt = time.perf_counter() - t0
        ok(L, rc)
        entries = int(L.pss_result_num_entries(res))
        nbytes = int(L.pss_result_offsets(res)[entries])
        L.pss_result_free(res)
        if i >= warmup:
            times.append(dt * 1e3)
    return {**spread(times, reps), 'entries': entries, 'bytes': nbytes}


def child(args):
    L = load(args.lib)
    out = {'lib': os.path.basename(args.lib)}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, 'words15.idx')
        blob, offs = write_index(L, p, args.queries)
        out['queries'] = len(offs) - 1

        def open_reader():
            h = ctypes.c_void_p()
            ok(L, L.pss_reader_open(p.encode(), 0, 0, 1, ctypes.byref(h)))
            return h

        h = open_reader()
        out['packed'] = timed(L, L.pss_reader_search_batch, h, blob, offs, args.warmup, args.reps)
        if args.ids:
            hbm0 = ctypes.c_uint64()
            ok(L, L.pss_reader_residency(h, ctypes.byref(hbm0), None, None))
            L.pss_reader_close(h)
            out['ids_by_shift'] = {}
            for shift in (8, 6, 7, 9, 10):
                os.environ['PSS_LINE_BLOCK_SHIFT'] = str(shift)
                builds = []
                for i in range(5):                          # a fresh reader each time: the first call builds all the tables
                    h = open_reader()
                    num = ctypes.c_uint64()
                    t0 = time.perf_counter()
                    ok(L, L.pss_reader_chunk_entries(h, None, None, 0, ctypes.byref(num)))
                    builds.append((time.perf_counter() - t0) * 1e3)
                    hbm = ctypes.c_uint64()
                    ok(L, L.pss_reader_residency(h, ctypes.byref(hbm), None, None))
                    if i < 4:                               # (the last one stays for the batch below)
                        L.pss_reader_close(h)
                leg = timed(L, L.pss_reader_search_ids_batch, h, blob, offs, args.warmup, args.reps)
                leg.update({'block_bytes': 1 << shift, 'table_bytes': int(hbm.value - hbm0.value),
                            'build_all_chunks_ms_first': round(builds[0], 4),
                            'build_all_chunks_ms_median_of_later': round(statistics.median(builds[1:]), 4),
                            'build_per_chunk_ms': round(statistics.median(builds[1:]) / CHUNKS, 4)})
                out['ids_by_shift'][str(shift)] = leg
                if shift == 8:      # the packed leg again, on the reader that now holds line tables
                    out['packed_after_ids'] = timed(L, L.pss_reader_search_batch, h, blob, offs, args.warmup, args.reps)
                L.pss_reader_close(h)
            out['ids'] = out['ids_by_shift']['8']
        else:
            L.pss_reader_close(h)
    print('IDS_PERF ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'entry_ids_vs_packed.json'))
    ap.add_argument('--parent-lib', default=None, help='libpss.so built from the parent commit (packed leg only)')
    ap.add_argument('--queries', type=int, default=20000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--rounds', type=int, default=3, help='alternations of the parent and this library')
    ap.add_argument('--timeout', type=int, default=240, help='seconds one child process may take')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--lib', default=os.path.join(ROOT, 'pysubstringsearch_amd', 'libpss.so'))
    ap.add_argument('--ids', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child(args)

    def run(lib, ids):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--lib', lib, '--queries', str(args.queries), '--warmup', str(args.warmup),
               '--reps', str(args.reps)] + (['--ids'] if ids else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:       # a leg that failed ends the measurement: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f'{os.path.basename(lib)}: child exited with {r.returncode}')
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('IDS_PERF ')][-1]
        return json.loads(line[len('IDS_PERF '):])

    out = {'what': 'search_batch_packed vs search_ids_batch, 15 chunks x 1 MiB of `words`, queries of 4 .. 8 bytes cut from the text; '
                   'host clock around the C call (ends in a stream synchronise), median / min / max over reps after warm-up; '
                   'runs alternate between the library of the parent commit and this one',
           'queries': args.queries, 'warmup': args.warmup, 'reps': args.reps, 'runs': []}
    for k in range(args.rounds):
        if args.parent_lib:
            out['runs'].append({'library': 'parent', **run(args.parent_lib, False)})
        out['runs'].append({'library': 'this', **run(args.lib, k == args.rounds - 1)})
    this = [r['packed']['median_ms'] for r in out['runs'] if r['library'] == 'this']
    parent = [r['packed']['median_ms'] for r in out['runs'] if r['library'] == 'parent']
    last = out['runs'][-1]
    out['summary'] = {'packed_median_ms_this': this, 'packed_median_ms_parent': parent,
                      'ids_median_ms': last['ids']['median_ms'], 'packed_median_ms_same_run': last['packed']['median_ms'],
                      'entries': last['ids']['entries'], 'ids_bytes': last['ids']['bytes'], 'packed_bytes': last['packed']['bytes'],
                      'line_tables_build_per_chunk_ms': last['ids']['build_per_chunk_ms'], 'line_table_bytes': last['ids']['table_bytes']}
    write_json(out, args.out)
    print(json.dumps(out['summary']))


if __name__ == '__main__':
    main()
