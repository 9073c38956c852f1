"""Compares two `rocprofv3 --kernel-trace` runs of tests/tools/rounds_check.py -- or, with --stages search, of
tests/tools/search_check.py -- (one per library): the dispatches must be the same in the same order, each as `kernel grid
workgroup lds`.

    python tests/tools/rounds_trace_diff.py <a_kernel_trace.csv> <b_kernel_trace.csv> [--stages rounds|search] [--per-queue]
                                            [--summary-a FILE] [--summary-b FILE]

Without --per-queue the dispatches of the whole process are ordered by start time (one stream: the side line off).  With it
they are compared queue by queue, the queues taken in the order of their first dispatch (the side line's helper stream
runs beside the main one, so the interleaving of the two is a race and the order inside each is not).
A summary file holds what fits a repository: the number of dispatches, the sha256 of the full sequence and the count per
kernel.  Exit code 0 = equal, and every stage of the driver was seen (STAGES: a stage is seen when a kernel's name starts
with it)."""
import argparse
import collections
import csv
import hashlib
import sys

STAGES = {}
STAGES['rounds'] = ('build_keys_kernel<true>', 'build_keys_kernel<false>', 'ht_insert_kernel', 'mid_msort_kernel', 'bg_merge_kernel', 'per_keys_kernel',
          'big_writeback_kernel', 'anc_select_kernel<true>', 'anc_select_kernel<false>', 'probe_repeats_kernel', 'isa_from_sa_kernel')
# the stages of a search batch (csrc/search.hip, Batch): run_fused, launch_interval, run_mid, pick_drivers, seed_drivers, and of
# run_general the hit scan, every branch of candidates() with the verify launcher's three ways under both folds, the counts
# tail and the emit tail
STAGES['search'] = ('search_block_kernel', 'search_small_kernel', 'search_interval_kernel', 'search_interval_group_kernel',
                    'search_interval_lane_kernel', 'anchor_edges_kernel', 'mid_hitoff_kernel', 'mid_hit_scans_kernel',
                    'terms_driver_kernel<true>', 'seed_union_kernel', 'terms_driver_kernel<false>', 'hit_bounds_kernel',
                    'mark_later_hits_kernel', 'anchored_hits_kernel', 'seed_hits_kernel', 'seed_dedupe_kernel', 'seqc_verify_kernel<true>',
                    'seqc_verify_kernel<false>', 'seq_verify_kernel<true>', 'seq_verify_kernel<false>', 'terms_verify_kernel<true>',
                    'terms_verify_kernel<false>', 'hit_lines_kernel<true>', 'hit_lines_kernel<false>', 'query_counts_kernel',
                    'emit_ids_kernel', 'emit_kernel')


def short(name):
    name = name.replace('pss::', '').replace('(anonymous namespace)::', '').replace('void ', '')
    depth = 0
    for i, c in enumerate(name):      # cut the argument list, keep the template arguments
        if c == '<':
            depth += 1
        elif c == '>':
            depth -= 1
        elif c == '(' and depth == 0:
            return name[:i]
    return name


def load(path, per_queue):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    queues = collections.OrderedDict()
    for r in rows:
        q = r.get('Queue_Id', '0') if per_queue else '0'
        queues.setdefault(q, []).append('%s grid %sx%sx%s wg %sx%sx%s lds %s' % (
            short(r['Kernel_Name']), r['Grid_Size_X'], r['Grid_Size_Y'], r['Grid_Size_Z'], r['Workgroup_Size_X'], r['Workgroup_Size_Y'],
            r['Workgroup_Size_Z'], r['LDS_Block_Size']))
    return list(queues.values())


def summary(queues, path):
    with open(path, 'w') as f:
        for k, seq in enumerate(queues):
            f.write('queue %d: %d dispatches, sha256 of the sequence %s\n' % (k, len(seq), hashlib.sha256('\n'.join(seq).encode()).hexdigest()))
        counts = collections.Counter(line.split(' grid ')[0] for seq in queues for line in seq)
        for name in sorted(counts):
            f.write('%8d  %s\n' % (counts[name], name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--per-queue', action='store_true')
    ap.add_argument('--stages', default='rounds', choices=sorted(STAGES))
    ap.add_argument('--summary-a')
    ap.add_argument('--summary-b')
    args = ap.parse_args()
    A, B = load(args.a, args.per_queue), load(args.b, args.per_queue)
    if args.summary_a:
        summary(A, args.summary_a)
    if args.summary_b:
        summary(B, args.summary_b)
    bad = 0
    if len(A) != len(B):
        print('queues: %d against %d' % (len(A), len(B)))
        bad += 1
    for k, (x, y) in enumerate(zip(A, B)):
        if x == y:
            print('queue %d: %d dispatches, the same in the same order' % (k, len(x)))
            continue
        bad += 1
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print('queue %d: %d against %d dispatches, first difference at %d:' % (k, len(x), len(y), first))
        for i in range(max(0, first - 2), min(first + 3, max(len(x), len(y)))):
            print('   %d  a: %s\n   %d  b: %s' % (i, x[i] if i < len(x) else '-', i, y[i] if i < len(y) else '-'))
    seen = set(line.split(' grid ')[0] for seq in B for line in seq)
    missing = [s for s in STAGES[args.stages] if not any(name.startswith(s) for name in seen)]
    print('stages missing from the trace:', missing if missing else 'none')
    sys.exit(1 if bad or missing else 0)


if __name__ == '__main__':
    main()
