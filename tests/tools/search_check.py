"""One line per search batch for a fixed list of readers, batches and switch settings: the sha256 over the result's counts,
offsets and bytes, the route bits and the hits / entries / result_bytes of last_stats (the clocks are left out).  Made to
be run twice in fresh processes, once per library (PSS_LIBPSS names the other one), and compared line for line: a change
to the host driver of the batched search (csrc/search.hip, Batch; csrc/search_layout.h) that keeps every decision and every
layout leaves the two outputs equal.  Under `rocprofv3 --kernel-trace` the same run is the record of its launches
(tests/tools/rounds_trace_diff.py --stages search).

    python tests/tools/search_check.py [--out FILE]

Readers: the edge corpus of tests/search_harness.py (a few hundred short entries) as one chunk and as three, in text order
and with order='sa'; the chunks of four cases of tests/search_fuzz_cases.py, handed over on the device.  Batches: every
kind of search -- plain, anchored, all-terms, glob, byte classes, each of the last three under icase, icase, near, edit --
in its three result forms (ids, packed text, counts), over 63, 64 and 65 rows whose term bytes add up to 31, 32 and 33
modulo 64; plain batches of 1, 40 and 3000 queries (the fused kernels, the mid pipeline, the general one) and a single
Reader.search; the six batches of every fuzz case.  Switches: none, then each search switch of the registry's "Fuzzed
with" column (tests/tools/README.md) by itself, with every value listed there.  Low-latency mode is left out: whether the
resident kernel answers depends on the clock."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from pysubstringsearch_amd import _ffi
from tests import search_fuzz_cases
from tests import search_harness as H
from tests.test_glob_class_gpu import CLASS, CLASS_ICASE

SWITCHES = [{}] + [{name: value} for name, values in (
    ('PSS_NO_SMALL_PATH', (1,)), ('PSS_NO_BLOCK_PATH', (1,)), ('PSS_NO_SEARCH_STAGE', (1,)), ('PSS_WAVE_SEARCH', (1,)),
    ('PSS_NO_GROUP_SEARCH', (1,)), ('PSS_NO_MID_PIPELINE', (1,)), ('PSS_NO_PINNED_RESULTS', (1,)), ('PSS_LANE_SEARCH_MIN', (1, 100000)),
    ('PSS_ICASE_SEED_LETTERS', (1, 2, 3, 4, 5, 6))) for value in values]
FOLDED = (H.ICASE, H.ICASE_ALL, H.ICASE_GLOB, CLASS_ICASE)
FUZZ_SEEDS = (3, 11, 29, 64)
_SET = set()


def set_env(**kv):
    """Exactly these switches, nothing left over from the batch before."""
    for k in _SET:
        os.environ.pop(k, None)
    _SET.clear()
    for k, v in kv.items():
        os.environ[k] = str(v)
        _SET.add(k)
    _ffi.lib.pss_reload_env()


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(b'%d:' % a.size)
        h.update(a.tobytes())
    return h.hexdigest()


def line(out, label, r, what):
    st = r.last_stats()
    print('%s sha256=%s route=%#x queries=%d hits=%d entries=%d result_bytes=%d' % (
        label, what, st['route'], st['queries'], st['hits'], st['entries'], st['result_bytes']), file=out, flush=True)


def forms(out, label, r, kind, batch):
    res = kind.ids(r, batch)
    line(out, label + ' ids', r, digest(res.counts, res.ids))
    pk = kind.packed(r, batch)
    line(out, label + ' packed', r, digest(pk.counts, pk.offsets, pk.data))
    line(out, label + ' counts', r, digest(np.array(kind.counts(r, batch), dtype=np.uint64)))


def edge_batches(lines):
    """{(rows, bytes modulo 64): {kind name: (kind, batch)}} over the triples of search_harness.edge_groups."""
    rng = np.random.default_rng(31 + 32 + 33)
    out = {}
    for rows in H.EDGE_ROWS:
        for mod in H.EDGE_BYTES:
            g = H.edge_groups(rng, lines, rows, mod)
            whole, budgets = [ab for _, _, ab in g], [i % 2 for i in range(len(g))]
            pairs, swapped = [[a, b] for a, b, _ in g], [(a.swapcase(), b.swapcase(), ab) for a, b, ab in g]
            out[rows, mod] = [
                (H.PLAIN, whole), (H.ANCHORED, (whole, [search_fuzz_cases.KINDS[i % 3] for i in range(len(g))])), (H.ALL_TERMS, pairs),
                (H.GLOB, H.edge_globs(g)), (CLASS, H.edge_globs(g, gap=b'?*')), (CLASS_ICASE, H.edge_globs(swapped, gap=b'?*')),
                (H.ICASE, [w.swapcase() for w in whole]), (H.ICASE_ALL, [[a, b] for a, b, _ in swapped]), (H.ICASE_GLOB, H.edge_globs(swapped)),
                (H.NEAR, (whole, budgets)), (H.EDIT, (whole, budgets))]
    return out


def edge_runs(out):
    lines, placements = H.edge_chunks()
    batches = edge_batches(lines)
    rng = np.random.default_rng(3000)
    many = [lines[int(i)][:int(rng.integers(1, 6))] or b'a' for i in rng.integers(0, len(lines), 3000)]
    for chunks in placements:
        for order in ('text', 'sa'):
            r = H.device_reader(chunks)
            r.set_result_order(order)
            where = 'edge chunks=%d order=%s' % (len(chunks), order)
            try:
                for sw in SWITCHES:
                    set_env(**sw)
                    name = ' '.join('%s=%s' % kv for kv in sw.items()) or 'default'
                    for (rows, mod), kinds in batches.items():
                        for kind, batch in kinds:
                            if 'PSS_ICASE_SEED_LETTERS' in sw and kind not in FOLDED:
                                continue
                            if sw and (rows, mod) != (64, 32) and kind is not H.PLAIN:      # (every edge under the defaults; the switches on one)
                                continue
                            forms(out, '%s %s rows=%d bytes=%d %s' % (where, name, rows, mod, kind.name), r, kind, batch)
                    if 'PSS_ICASE_SEED_LETTERS' in sw:
                        continue
                    for n in (1, 40, 3000):
                        forms(out, '%s %s plain n=%d' % (where, name, n), r, H.PLAIN, many[:n])
                    got = r.search(many[7].decode())
                    line(out, '%s %s search' % (where, name), r, digest(np.frombuffer('\n'.join(got).encode(), np.uint8)))
            finally:
                r.close()


def fuzz_runs(out):
    for seed in FUZZ_SEEDS:
        case = search_fuzz_cases.make_case(seed)
        set_env(**case.switches)
        r = H.device_reader(case.chunks)
        try:
            for name, kind, batch_of in H.FUZZ_BATCHES:
                forms(out, 'fuzz seed=%d chunks=%d %s' % (seed, len(case.chunks), name), r, kind, batch_of(case))
        finally:
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    out = open(args.out, 'w') if args.out else sys.stdout
    print('# library %s' % os.path.basename(os.path.dirname(_ffi.LIB_PATH)), file=sys.stderr)
    edge_runs(out)
    fuzz_runs(out)
    set_env()
    if args.out:
        out.close()


if __name__ == '__main__':
    main()
