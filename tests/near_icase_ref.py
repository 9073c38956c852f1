"""Brute-force reference of the search within k mismatches and within k edits UNDER ASCII CASE FOLDING (include/pss.h,
pss_reader_search_near_icase_batch), on top of tests/near_ref.py and tests/edit_ref.py: no suffix array, no pieces and no
seeds in what decides a match.

Both sides are folded -- bytes.lower folds A .. Z alone, which is exactly the contract -- and then the existing window
count (near_ref) or Sellers scan (edit_ref) runs over the folded entries with the folded pattern.  A pattern that holds a
newline matches nothing.  ordered_ids states the order contract and piece_hits what the `hits` of a batch are pinned to;
only those two and the rule_set_lines functions know the seed rule, restated here (`seeds`): the pieces are near's, a piece
is looked up through the spellings, ascending, of its SEED -- its longest window with at most f ASCII letters, the leftmost
on a tie --, and f = min(letters, CAP[k]) so that a pattern has at most 64 queries.  CPU only;
tests/test_near_icase_gpu.py compares every pattern of every case."""
import itertools
import typing

import numpy as np

from tests import edit_ref
from tests.edit_ref import EditRef
from tests.near_ref import NearRef, pieces
from tests.search_ref import occurrences

CAP = (6, 5, 4, 4)              # the largest f with (k + 1) * 2**f <= 64
LETTERS = 5                     # the default of PSS_ICASE_SEED_LETTERS


def is_letter(b: int) -> bool:
    return 0x41 <= b <= 0x5a or 0x61 <= b <= 0x7a


def fold_seed(piece: bytes, f: int) -> typing.Tuple[int, int]:
    """(offset, length) of the longest window of piece with at most f ASCII letters, the leftmost on a tie."""
    best = (0, 0)
    for a in range(len(piece)):
        letters, b = 0, a
        while b < len(piece) and letters + is_letter(piece[b]) <= f:
            letters += is_letter(piece[b])
            b += 1
        if b - a > best[1]:
            best = (a, b - a)
    return best


def spellings(seed: bytes) -> typing.List[bytes]:
    """Every spelling of seed (each ASCII letter in either case), ascending bytewise."""
    choices = [(bytes([b & ~0x20]), bytes([b | 0x20])) if is_letter(b) else (bytes([b]),) for b in seed]
    return sorted(b''.join(c) for c in itertools.product(*choices))


def seeds(pattern: bytes, k: int, letters: int = LETTERS) -> typing.List[typing.Tuple[int, int, bytes]]:
    """[(piece, pos, bytes)]: the seed queries of pattern at budget k in the order of the search -- piece-major, the
    spellings of one piece ascending; pos is the seed's position inside the pattern."""
    f = min(letters, CAP[k])
    out = []
    for j, (off, piece) in enumerate(pieces(pattern, k)):
        so, sl = fold_seed(piece, f)
        out += [(j, off + so, s) for s in spellings(piece[so:so + sl])]
    return out


def _lines(text: bytes):
    nl = [i for i, b in enumerate(text) if b == 0x0A]

    def bounds(d):
        line = int(np.searchsorted(nl, d, side='left'))
        return line, (nl[line - 1] + 1 if line else 0), (nl[line] if line < len(nl) else len(text))
    return bounds


def rule_set_lines(text: bytes, pattern: bytes, k: int, letters: int = LETTERS) -> typing.List[int]:
    """Mismatches.  The lines of ONE chunk text that the engine's rule set keeps, in the engine's order -- DESIGN.md 4.19
    restated hit by hit: every exact occurrence di of every seed query (piece j, position pos), query-major and in suffix
    order inside a query, is a hit; with m = di - pos it survives iff the window [m, m + L) lies in the chunk, piece j is
    fold-equal in it over its whole length (1), no piece j' < j is (2), the window differs from the pattern in at most k
    bytes under fold (3), it lies in di's entry (4), and no window within budget starts in [entry start, m)."""
    if b'\n' in pattern:
        return []
    low, P = text.lower(), pattern.lower()
    n, L = len(text), len(pattern)
    p, t = np.frombuffer(P, np.uint8), np.frombuffer(low, np.uint8)
    miss = lambda s: int((t[s:s + L] != p).sum())
    cut, bounds, kept = pieces(P, k), _lines(text), []
    for j, pos, q in seeds(pattern, k, letters):
        for di in sorted(occurrences(text, q).tolist(), key=lambda d: text[d:]):
            m = di - pos
            if m < 0 or m + L > n:
                continue
            if any((low[m + o:m + o + len(x)] == x) != (i == j) for i, (o, x) in enumerate(cut[:j + 1])):
                continue
            line, start, end = bounds(di)
            if miss(m) > k or m < start or m + L > end:
                continue
            if any(miss(s) <= k for s in range(start, m)):
                continue
            kept.append(line)
    return kept


def edit_rule_set_lines(text: bytes, pattern: bytes, k: int, letters: int = LETTERS) -> typing.List[int]:
    """Edits.  As above for DESIGN.md 4.19's second rule set: a hit di of a seed query (piece j at off_j, position pos)
    names the candidate position d = di - (pos - off_j); d < 0 or a piece past n rejects it; it is kept iff piece j is
    fold-equal at d, the candidate (d, j) stands under fold (tests/edit_ref.stands over the folded text and pattern), no
    piece j' < j is fold-exact at d and stands there, and no candidate stands at a d' in [entry start, d)."""
    if b'\n' in pattern:
        return []
    low, P = text.lower(), pattern.lower()
    cut, bounds, kept, memo = pieces(P, k), _lines(text), [], {}

    def st(j, d):
        if (j, d) not in memo:
            off, piece = cut[j]
            memo[j, d] = low[d:d + len(piece)] == piece and edit_ref.stands(low, P, k, off, piece, d)
        return memo[j, d]

    for j, pos, q in seeds(pattern, k, letters):
        off, piece = cut[j]
        for di in sorted(occurrences(text, q).tolist(), key=lambda d: text[d:]):
            d = di - (pos - off)
            if d < 0 or d + len(piece) > len(text):
                continue
            if not st(j, d) or any(st(i, d) for i in range(j)):
                continue
            line, start, _ = bounds(d)
            if any(st(i, e) for e in range(start, d) for i in range(len(cut))):
                continue
            kept.append(line)
    return kept


class _FoldedRef:
    """What the two references share: `inner`, the exact-byte reference over the folded chunks, answers the folded
    pattern; the entries' text, the order keys and the hits come from the chunks as they are."""
    inner_cls: type = None
    letters = LETTERS

    def _fold_init(self, texts, indices):
        self._inner = self.inner_cls([bytes(t).lower() for t in texts], indices)
        self._ordered_fold = {}

    def ordered_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """The ids in the order the engine states: chunk-major; inside a chunk by the piece index j of the entry's kept hit,
        then by query and in suffix-array order inside a query -- the spellings of a seed ascend bytewise, so both are the
        order of the suffixes text[s:] of the UNFOLDED text at the occurrence s of the kept hit's seed."""
        pattern = bytes(pattern)
        if (pattern, k) not in self._ordered_fold:
            out = []
            if b'\n' not in pattern:
                P = pattern.lower()
                sd = {j: pos for j, pos, _ in seeds(pattern, k, self.letters)}
                for ch, low, entries in zip(self.chunks, self._inner.chunks, self._inner._true):
                    keyed, start = [], 0
                    for line, e in enumerate(entries):
                        at = self._kept(low.text, e, start, P, k, sd)
                        if at is not None:
                            keyed.append((at[0], ch.text[at[1]:], (ch.index << 32) | line))
                        start += len(e) + 1
                    out += [i for _, _, i in sorted(keyed)]
            self._ordered_fold[pattern, k] = np.array(out, dtype=np.uint64)
        return self._ordered_fold[pattern, k]

    def piece_hits(self, pattern: bytes, k: int) -> int:
        """Exact occurrences of every seed query over every chunk: the candidates.  A pattern that holds a newline is not
        looked up at all."""
        pattern = bytes(pattern)
        if b'\n' in pattern:
            return 0
        return sum(int(occurrences(ch.text, q).size) for ch in self.chunks for _, _, q in seeds(pattern, k, self.letters))


class NearIcaseRef(_FoldedRef, NearRef):
    inner_cls = NearRef

    def __init__(self, texts, indices=None):
        NearRef.__init__(self, texts, indices)
        self._fold_init(texts, indices)

    def search_near_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """Ids of the entries that hold pattern within k mismatches under fold, ascending."""
        return self._inner.search_near_ids(bytes(pattern).lower(), k)

    @staticmethod
    def _kept(low, e, start, P, k, sd):
        """(j, s): the first fold-exact piece of the entry's leftmost window within budget, and where its seed stands."""
        from tests.near_ref import near_starts
        at = near_starts(e, P, k) if len(e) >= len(P) else ()
        if not len(at):
            return None
        m = int(at[0])
        cut = pieces(P, k)
        j, off = next((j, off) for j, (off, piece) in enumerate(cut) if e[m + off:m + off + len(piece)] == piece)
        return j, start + m + sd[j]


class EditIcaseRef(_FoldedRef, EditRef):
    inner_cls = EditRef

    def __init__(self, texts, indices=None):
        EditRef.__init__(self, texts, indices)
        self._fold_init(texts, indices)

    def search_edit_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """Ids of the entries that hold pattern within k edits under fold, ascending."""
        return self._inner.search_edit_ids(bytes(pattern).lower(), k)

    def _kept(self, low, e, start, P, k, sd):
        """(j, s): the entry's kept candidate (d, j) under fold, and where the seed of piece j stands."""
        if self._inner.distance(e, P) > k:
            return None
        d, j = edit_ref.kept_candidate(low, P, k, start, start + len(e))
        return j, d + sd[j] - pieces(P, k)[j][0]
