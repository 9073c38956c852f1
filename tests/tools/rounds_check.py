"""One line per build for a fixed list of small texts under each switch setting that steers the rounds: the sha256 of the
suffix array and every integer field of pss_sa_stats (the clocks -- ms_*, anchor_ms -- are left out).  Made to be run
twice in fresh processes, once per library (PSS_LIBPSS names the other one), and compared line for line: a change to the
host driver of the rounds (csrc/sa_refine_impl.h, csrc/anchor_driver_impl.h) that keeps every decision leaves the two
outputs equal.  Under `rocprofv3 --kernel-trace` the same run is the record of its launches (tests/tools/rounds_trace_diff.py).

    python tests/tools/rounds_check.py [--side 0|1|both] [--out FILE]

Texts: sa_edge_texts.tier_case for TIER_KS x three shapes x TIER_VARIANTS of tests/test_sa_edges_gpu.py; the anchor
suite's texts (tiled, ladder, on the cap, the levels case at 2^18) with PSS_ANCHOR=1 and PSS_ANCHOR_SIDE=0 / 1; two
run-length and two periodic texts of rle_texts.py with PSS_RLE=1; gen_corpus kinds 1, 5, 6, 7 at 2^20 by default, under
PSS_MODE=dense and under PSS_PERIODIC=0; kind 0 under short keys (few ties: the sparse mode's hash table and key search);
the probe's texts of tests/test_sa_edges_gpu.py; kinds 5 and 6 without the anchor round.  Every build is cold
(PSS_SA_COLD): no line depends on the one before it.
"""
import argparse
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from pysubstringsearch_amd import _ffi
from tests import anchor_texts as A
from tests import rle_texts as R
from tests import sa_edge_texts as E
from tests.test_anchor_edges_gpu import COMMON, TINY
from tests.test_sa_edges_gpu import TIER_VARIANTS
from tests.util import gen_corpus, sa_device

INT_FIELDS = [name for name, ctype in _ffi.SaStats._fields_ if ctype in (ctypes.c_uint32, ctypes.c_uint64)]
INT_ARRAYS = [name for name, ctype in _ffi.SaStats._fields_ if getattr(ctype, '_type_', None) is ctypes.c_uint64 and hasattr(ctype, '_length_')]
_SET = set()


def set_env(**kv):
    """Exactly these switches, nothing left over from the previous build."""
    for k in _SET:
        os.environ.pop(k, None)
    _SET.clear()
    for k, v in kv.items():
        os.environ[k] = str(v)
        _SET.add(k)


def line(label, t, out):
    st = {}
    sa = sa_device(np.ascontiguousarray(t), st, flags=_ffi.SA_COLD)
    fields = ['%s=%d' % (k, int(st[k])) for k in INT_FIELDS]
    fields += ['%s=%s' % (k, ','.join(str(int(x)) for x in st[k])) for k in INT_ARRAYS]
    text = '%s n=%d sha256=%s %s' % (label, t.size, hashlib.sha256(np.ascontiguousarray(sa).tobytes()).hexdigest(), ' '.join(fields))
    print(text, file=out, flush=True)
    return st


def tier_builds(out):
    texts = {(k, shape): E.tier_case(k, shape) for shape in ('plain', 'second', 'crowded') for k in E.TIER_KS}
    for variant, env in TIER_VARIANTS.items():
        set_env(**env)
        for (k, shape), t in texts.items():
            line('tier %d %s %s' % (k, shape, variant), t, out)


def anchor_builds(out, side):
    cases = []
    for alpha in sorted(A.ALPHABETS):
        for n in A.TILED_NS:
            cases.append(('tiled %d %d' % (n, alpha), A.tiled(n, alpha), TINY if n <= 66 else {}, None))
        cases.append(('tiled 8193 %d omega 12' % alpha, A.tiled(8193, alpha), {}, 12))
    ladder = A.ladder()
    cases += [('ladder', ladder, {}, None), ('ladder omega 33', ladder, {}, 33)]
    for div in A.CAP_DIVS:
        omega, on, over = A.on_the_cap(div, A.CAP_W)
        cases += [('cap %d on' % div, on, dict(PSS_ANCHOR_CAP_DIV=div), omega), ('cap %d over' % div, over, dict(PSS_ANCHOR_CAP_DIV=div), omega)]
    for alpha in A.DEEP_ALPHAS:
        deep = A.deep(A.DEEP_N, alpha)
        cases += [('deep %d' % alpha, deep, {}, None), ('deep %d periodic 0' % alpha, deep, dict(PSS_PERIODIC=0), None)]
    for label, t, env, forced in cases:
        env = dict(COMMON, PSS_ANCHOR_SIDE=side, **env)
        if forced:
            env['PSS_ANCHOR_OMEGA'] = forced
        set_env(**env)
        st = line('anchor side=%d %s' % (side, label), t, out)
        if side == 1 and st['anchor_side'] not in (1, 2):
            print('# side line not started: %s' % label, file=out, flush=True)


def rle_builds(out):
    set_env(PSS_RLE=1, PSS_PERIOD=0)
    for k in (513, 4097):
        line('rle tier %d' % k, R.tier_case(k), out)
    set_env(PSS_RLE=1)
    for where in ('16k', 'last'):
        line('periodic extent %s' % where, R.extent_case(where), out)


def corpus_builds(out):
    for kind in (1, 5, 6, 7):
        t = gen_corpus(kind, 1 << 20)
        for name, env in (('default', {}), ('dense', dict(PSS_MODE='dense')), ('periodic0', dict(PSS_PERIODIC=0))):
            set_env(**env)
            line('corpus %d %s' % (kind, name), t, out)
    # few ties: the sparse mode (hash table, key search) -- a key of 6 symbols leaves `lines` fewer than n / 1024 ties, one
    # of 5 fewer than n / 16, which the forced mode still takes
    lines = gen_corpus(0, 1 << 20)
    for name, env in (('default', {}), ('key6', dict(PSS_KEY_CHARS=6)), ('key5 sparse', dict(PSS_KEY_CHARS=5, PSS_MODE='sparse'))):
        set_env(**env)
        line('corpus 0 %s' % name, lines, out)
    # the probe of the ties (tests/test_sa_edges_gpu.py: _probe_base), and its verdict turned into "no text round"
    probed = [('planted600', E.switch_planted()), ('corpus 6', gen_corpus(6, 1 << 20)), ('corpus 7', gen_corpus(7, 1 << 20))]
    for name, env in (('probe', {}), ('probe skip 0', dict(PSS_PROBE_SKIP_PCT=0))):
        set_env(PSS_ANCHOR=1, PSS_ANCHOR_MIN_OMEGA=3, **env)
        for label, t in probed:
            line('%s %s' % (label, name), t, out)
    # repeats without the anchor round: rank rounds that go global
    set_env(PSS_ANCHOR=0)
    line('corpus 5 anchor0', gen_corpus(5, 1 << 20), out)
    set_env(PSS_ANCHOR=0, PSS_PERIODIC=0, PSS_BIG_MERGE=0)
    line('corpus 6 anchor0 chained', gen_corpus(6, 1 << 20), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', default='both', choices=['0', '1', 'both'], help='the anchor texts with PSS_ANCHOR_SIDE=0, =1 or both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    out = open(args.out, 'w') if args.out else sys.stdout
    print('# library %s' % os.path.basename(os.path.dirname(_ffi.LIB_PATH)), file=sys.stderr)
    tier_builds(out)
    for side in ((0, 1) if args.side == 'both' else (int(args.side),)):
        anchor_builds(out, side)
    rle_builds(out)
    corpus_builds(out)
    set_env()
    if args.out:
        out.close()


if __name__ == '__main__':
    main()
