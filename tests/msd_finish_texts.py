"""Texts for tests/test_msd_finish_gpu.py and a numpy model of what msd_finish_kernel (msd_sort.hip) must do with them.

The MSD sort leaves suffixes tied that share its key: key_chars symbols, code_bits each, without the lowest `drop` bits.
The finishing kernel settles a tied group of g <= FIN_MAX members when ONE more 64-bit text key -- `ks` symbols from
symbol h0 on, h0 = the whole symbols the sort key compared -- is different for every member; every other group goes to
the rounds whole.  The model restates the key format (sa_build.hip) and the rule, so that a test can say exactly how many
suffixes the kernel must report as finished and how many it must leave, and can check that a planted group is what the
case is about (its size at depth h0, the symbol at which its members first differ)."""
import numpy as np

FIN_MAX = 4          # msd_sort.hip
NL = 10
LEAD = 0xF5          # larger than every other byte of a text: suffixes that start with it end the suffix array


class Format:
    """Key format of the MSD sort for a text of n bytes with sigma distinct byte values (sa_build.hip, msd_sort.hip:
    msd_max_key_bits), for PSS_MSD_KEY_CAP = cap and PSS_MSD_PARTIAL_SYMBOL = partial."""

    def __init__(self, n, sigma, cap=48, partial=False, lsd=True):
        assert 2 <= sigma < 256
        self.b = b = sigma.bit_length()                    # codes 0 .. sigma
        kmax = min(64 // b, 16)
        ib = max(1, (n - 1).bit_length())
        most = min(64 + 10 - (6 if lsd else 11) - ib + 10, 64 + 10 - ib)
        kb = min(most, max(cap, 21))
        kc = min(-(-kb // b) if partial else kb // b, kmax)
        drop = kc * b - kb
        if drop < 0 or kc <= 1:
            kb, drop = kc * b, 0
        self.kc, self.kb, self.drop = kc, kb, drop
        self.h0 = kc - 1 if drop else kc
        self.ks = kmax                                     # symbols of the extra key


def codes_of(t):
    present = np.unique(t)
    lut = np.zeros(256, np.uint64)
    lut[present] = np.arange(1, present.size + 1, dtype=np.uint64)
    return np.concatenate([lut[t], np.zeros(96, np.uint64)])        # code 0 past the end


def _pack(codes, n, start, count, b):
    key = np.zeros(n, np.uint64)
    for j in range(count):
        key = (key << np.uint64(b)) | codes[start + j:start + j + n]
    return key


class Model:
    """Groups of a text under a format: size[i] = members of suffix i's group after the sort, finished[i] = the kernel
    settles it; n_finished / n_left = suffixes settled / left tied for the rounds."""

    def __init__(self, t, f):
        t = np.ascontiguousarray(t, dtype=np.uint8)
        n = t.size
        assert f.kc * f.b <= 64 and f.ks * f.b <= 64
        self.codes = codes = codes_of(t)
        key = _pack(codes, n, 0, f.kc, f.b) >> np.uint64(f.drop)
        ext = _pack(codes, n, f.h0, f.ks, f.b)
        order = np.lexsort((ext, key))
        ks, es = key[order], ext[order]
        head = np.r_[True, ks[1:] != ks[:-1]]
        gid = np.cumsum(head) - 1
        size = np.bincount(gid)
        dup = np.r_[False, ~head[1:] & (es[1:] == es[:-1])]
        has_dup = np.bincount(gid, weights=dup) > 0
        tied = size > 1
        fin = tied & (size <= FIN_MAX) & ~has_dup
        self.n_finished = int(size[fin].sum())
        self.n_left = int(size[tied & ~fin].sum())
        self.size = np.empty(n, np.int64)
        self.size[order] = size[gid]
        self.finished = np.empty(n, bool)
        self.finished[order] = fin[gid]
        self.slot = np.empty(n, np.int64)                 # a group's slots are final; inside it the order is the extra key's
        self.slot[order] = np.arange(n)

    def first_difference(self, i, j):
        """Symbol (0-based) at which suffixes i and j first differ, code 0 past the end."""
        a, b = self.codes[i:i + 90], self.codes[j:j + 90]
        d = np.nonzero(a != b)[0]
        assert d.size
        return int(d[0])


def background(rng, n, alpha):
    """n bytes: alpha byte values at random, '\\n' at the end (alpha + 1 distinct values)."""
    t = rng.integers(40, 40 + alpha, n).astype(np.uint8)
    t[-1] = NL
    return t


def plant(t, rng, copies, taken):
    """Writes every byte string of `copies` at a place of its own (not the text's ends, no overlap with `taken` --
    a list of (start, end) that grows); returns the places."""
    n = t.size
    at = []
    for c in copies:
        c = np.frombuffer(bytes(c), np.uint8)
        for _ in range(1000):
            p = int(rng.integers(64, n - 256))
            if all(p + c.size + 32 <= a or p >= e + 32 for a, e in taken):
                break
        else:
            raise AssertionError('no room')
        t[p:p + c.size] = c
        taken.append((p, p + c.size))
        at.append(p)
    return at


def word(rng, alpha, length):
    return bytes(rng.integers(40, 40 + alpha, length).astype(np.uint8))


def distinct_symbols(rng, alpha, count):
    return [bytes([40 + int(x)]) for x in rng.permutation(alpha)[:count]]
