"""CPU model of the bins of msd_local_fast_kernel (msd_sort.hip) on the `lines` corpus: how long the bin is that an element
of a real tile finds itself in, for a number of bin bits and a ranking window W.  Plain numpy, no GPU.

    python tests/tools/local_bins_model.py [logn=29] [bits:W ...]        (default 12:8 13:8 13:7 13:6)

The text is pss_gen_corpus(lines, 2^logn).  Its joint buckets are counted in blocks; the tile plan is the real one
(tests/sa_edge_texts.py: tile_heads, LSD order); the tiles looked at are all those of ONE region of the first digit, the
one that holds the middle of the suffix array -- consecutive tiles, about 2^logn / 400 elements.  For every tile the local
key is [bucket inside the tile | the key bits below the bucket], as in tests/local_rows_texts.py: View.slow_tiles, and
the bin its top `bits` bits.  Per (bits, W) and per kind of tile (by its number of buckets):

    mean    bin length seen by an element (sum of len^2 / sum of len)
    past    share of elements in a bin longer than W (they finish in the ranking's loop)
    waves   share of waves -- 64 consecutive positions of a tile in bin order, as the ranking runs -- with such an element:
            the whole wave waits for the loop
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from pysubstringsearch_amd import _ffi  # noqa: E402
from tests import msd_finish_texts as F  # noqa: E402
from tests import sa_edge_texts as E  # noqa: E402

BLOCK = 1 << 22
WAVE = 64


def keys_in_blocks(t, f):
    """Yields the sort key of every suffix, BLOCK positions at a time."""
    present = np.unique(t[:1 << 24])
    assert np.array_equal(present, np.unique(t[-(1 << 20):]))          # (the generator's alphabet shows in any stretch)
    lut = np.zeros(256, np.uint64)
    lut[present] = np.arange(1, present.size + 1, dtype=np.uint64)
    n = t.size
    for s in range(0, n, BLOCK):
        m = min(BLOCK, n - s)
        codes = lut[t[s:min(n, s + m + f.kc)]]
        codes = np.concatenate([codes, np.zeros(m + f.kc - codes.size, np.uint64)])
        yield F._pack(codes, m, 0, f.kc, f.b) >> np.uint64(f.drop)


def model(logn, variants):
    n = 1 << logn
    t = np.empty(n, np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus(_ffi.CORPUS_LINES, t.ctypes.data, n, 0))
    sigma = int(np.unique(t[:1 << 24]).size)
    f = F.Format(n, sigma)
    rem = f.kb - 20
    hist = np.zeros(1 << 20, np.int64)
    for key in keys_in_blocks(t, f):
        hist += np.bincount((key >> np.uint64(rem)).astype(np.int64), minlength=1 << 20)
    numbers = np.flatnonzero(hist)
    sizes = hist[numbers]
    start = np.concatenate([[0], np.cumsum(sizes)])
    head = E.tile_heads(numbers, sizes, n, True)
    d = int(numbers[np.searchsorted(start, n // 2, side='right') - 1] >> 10)        # the first digit in the middle of the array
    inside = numbers >> 10 == d
    k0, k1 = int(np.flatnonzero(inside)[0]), int(np.flatnonzero(inside)[-1]) + 1
    assert head[k0] and (k1 == len(numbers) or head[k1])                           # a tile never crosses a first digit
    keys = np.sort(np.concatenate([key[key >> np.uint64(rem + 10) == np.uint64(d)] for key in keys_in_blocks(t, f)]))
    assert keys.size == start[k1] - start[k0]
    # the tiles of the region and the local key of every element
    tag = E.lsd_numbers(numbers)[k0:k1] & (E.MSD_RAW_TAG_SPAN - 1)
    h = head[k0:k1]
    first = np.flatnonzero(h)
    last = np.append(first[1:], k1 - k0) - 1
    nb = tag[last] - tag[first] + 1
    seg = np.array([int(x - 1).bit_length() for x in nb])
    tile_of_bucket = np.cumsum(h) - 1
    rel = (tag - tag[first][tile_of_bucket]).astype(np.uint64)
    sz = sizes[k0:k1]
    tile = np.repeat(tile_of_bucket, sz)
    local = (np.repeat(rel, sz) << np.uint64(rem)) | (keys & np.uint64((1 << rem) - 1))
    e0 = (start[k0:k1][first] - start[k0])
    counts = np.diff(np.append(e0, keys.size))
    pos = np.arange(keys.size) - e0[tile]
    wave = tile * (8192 // WAVE) + pos // WAVE
    n_waves = np.unique(wave).size
    buckets = np.diff(np.append(first, k1 - k0))                                   # non-empty buckets per tile
    print(f'lines n=2^{logn}: sigma {sigma}, {f.b}-bit codes, key {f.kc} symbols = {f.kb} bits, {rem} below the bucket; '
          f'{len(numbers)} non-empty joint buckets, {int(head.sum())} tiles')
    print(f'region: first digit {d}, {keys.size} elements in {len(first)} consecutive tiles '
          f'({int((buckets == 1).sum())} of one bucket, {int((buckets == 2).sum())} of two, {int((buckets > 2).sum())} of more), '
          f'{counts.min()}..{counts.max()} elements, tag spans {nb.min()}..{nb.max()}')
    kinds = [('all tiles', np.ones(len(first), bool)), ('one bucket', nb == 1), ('tag span 2', nb == 2), ('tag span 3+', nb > 2)]
    print(f'{"bits":>4} {"W":>2} {"tiles":<12} {"tiles":>6} {"elements":>9} {"used bins/tile":>14} {"mean":>6} {"past":>8} {"waves":>8}')
    out = {}
    for bits, w in variants:
        bins = local >> np.maximum(0, rem + seg[tile] - bits).astype(np.uint64)
        _, inv, cnt = np.unique(tile.astype(np.uint64) << np.uint64(32) | bins, return_inverse=True, return_counts=True)
        length = cnt[inv]
        for name, pick in kinds:
            if not pick.any():
                continue
            el = pick[tile]
            ln = length[el]
            past = ln > w
            waves = np.unique(wave[el]).size
            loop = np.unique(wave[el][past]).size
            used = np.unique((tile[el].astype(np.uint64) << np.uint64(32)) | bins[el]).size / int(pick.sum())
            out[(bits, w, name)] = (float(ln.mean()), float(past.mean()), loop / waves)
            print(f'{bits:>4} {w:>2} {name:<12} {int(pick.sum()):>6} {int(el.sum()):>9} {used:>14.0f} {ln.mean():>6.2f} '
                  f'{100 * past.mean():>7.2f}% {100 * loop / waves:>7.2f}%')
    assert n_waves >= keys.size // WAVE
    return out


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 29
    variants = [tuple(int(x) for x in a.split(':')) for a in sys.argv[2:]] or [(12, 8), (13, 8), (13, 7), (13, 6)]
    model(logn, variants)


if __name__ == '__main__':
    main()
