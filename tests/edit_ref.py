"""Brute-force reference of the search within k edits (include/pss.h, pss_reader_search_edit_batch), on top of the
entry-id reference of tests/entry_id_ref.py: no suffix array and no pieces in what decides a match.

Per chunk every entry's TRUE bytes are enumerated (tests/glob_ref.true_entries: text[start : newline], or text[start : n]
for an unterminated last entry) and an entry matches pattern p within k when SOME SUBSTRING of those bytes has
Levenshtein distance <= k to p: a plain Sellers scan, D[0][j] = 0, the least value of the last row over the entry.  The
substrings of an entry never reach over its newline, because the entry's bytes hold none.  A pattern that holds a newline
matches nothing.  ordered_ids states the order contract and piece_hits what the `hits` of a batch are pinned to; only
those two and rule_set_lines know the pieces (tests/near_ref.pieces: the cut is near's).  CPU only;
tests/test_edit_gpu.py compares every pattern of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef
from tests.glob_ref import true_entries
from tests.near_ref import pieces
from tests.search_ref import occurrences


def sellers(entry: bytes, pattern: bytes) -> int:
    """The least lev(w, pattern) over the substrings w of entry (the empty one included: at most len(pattern)): the plain
    Sellers scan, column by column over the entry, D[0][j] = 0 (a match starts anywhere) and D[i][0] = i."""
    L = len(pattern)
    col = list(range(L + 1))
    best = L
    for c in entry:
        diag, left = 0, 0                       # D[0][j - 1] and D[0][j]
        for i in range(1, L + 1):
            up = col[i]                         # D[i][j - 1]
            left = min(diag + (pattern[i - 1] != c), up + 1, left + 1)
            diag, col[i] = up, left
        if left < best:
            best = left
    return best


def prefix_lev(t: bytes, p: bytes) -> int:
    """The least lev(t[:x], p) over x in 0 .. len(t): the full table, no band."""
    row = list(range(len(t) + 1))               # lev(t[:x], '') = x
    for i, c in enumerate(p, 1):
        new = [i]
        for x in range(1, len(t) + 1):
            new.append(min(row[x - 1] + (t[x - 1] != c), row[x] + 1, new[x - 1] + 1))
        row = new
    return min(row)


def walls(text: bytes, d: int, end: int) -> typing.Tuple[int, int]:
    """(a, b): the text around the piece text[d:end] up to the walls -- a byte 0x0A or an index outside [0, n) --,
    walked byte by byte as the kernel walks it: text[a:d] and text[end:b] are what the two sides may take."""
    a, b = d, end
    while a > 0 and text[a - 1] != 0x0A:
        a -= 1
    while b < len(text) and text[b] != 0x0A:
        b += 1
    return a, b


def stands(text: bytes, pattern: bytes, k: int, off: int, piece: bytes, d: int) -> bool:
    """Does the candidate (piece at off inside pattern, exact at text offset d) stand?  lc + rc <= k, the left side
    within k and the right side within k - lc."""
    assert text[d:d + len(piece)] == piece
    a, b = walls(text, d, d + len(piece))
    lc = prefix_lev(text[a:d][::-1], pattern[:off][::-1])
    if lc > k:
        return False
    return prefix_lev(text[d + len(piece):b], pattern[off + len(piece):]) <= k - lc


def kept_candidate(text: bytes, pattern: bytes, k: int, start: int, end: int) -> typing.Optional[typing.Tuple[int, int]]:
    """(d, j) of the one hit kept for the entry text[start:end]: the standing candidate with the smallest d and, among
    equal d, the smallest j; None where no candidate stands."""
    cut = pieces(pattern, k)
    for d in range(start, end):
        for j, (off, piece) in enumerate(cut):
            if d + len(piece) <= end and text[d:d + len(piece)] == piece and stands(text, pattern, k, off, piece, d):
                return d, j
    return None


def rule_set_lines(text: bytes, pattern: bytes, k: int) -> typing.List[int]:
    """The lines of ONE chunk text that the engine's rule set keeps, in the engine's order -- the rules of DESIGN.md
    4.17 restated hit by hit, so that they can be held against the Sellers scan above without a GPU: every exact
    occurrence d of every piece j, piece-major and in suffix order inside a piece, is a candidate; it is kept iff it
    stands (both sides walled by newlines and the chunk's ends), no piece j' < j is exact at d and stands there, and no
    candidate stands at a d' in [entry start, d)."""
    if b'\n' in pattern:
        return []
    nl = [i for i, b in enumerate(text) if b == 0x0A]
    cut, kept = pieces(pattern, k), []
    memo = {}

    def st(j, d):
        if (j, d) not in memo:
            off, piece = cut[j]
            memo[j, d] = text[d:d + len(piece)] == piece and stands(text, pattern, k, off, piece, d)
        return memo[j, d]

    for j, (off, piece) in enumerate(cut):
        for d in sorted(occurrences(text, piece).tolist(), key=lambda x: text[x:]):
            if not st(j, d) or any(st(i, d) for i in range(j)):
                continue
            start, _ = walls(text, d, d + len(piece))
            if any(st(i, e) for e in range(start, d) for i in range(len(cut))):
                continue
            kept.append(int(np.searchsorted(nl, d, side='left')))
    return kept


class EditRef(IdRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = [true_entries(ch.text, ch.nl) for ch in self.chunks]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._true, self.chunks))
        self._ids, self._ordered, self._dist = {}, {}, {}    # (computed once per (pattern, k): the tests of one index share them)

    def distance(self, entry: bytes, pattern: bytes) -> int:
        if (entry, pattern) not in self._dist:
            self._dist[entry, pattern] = sellers(entry, pattern)
        return self._dist[entry, pattern]

    def search_edit_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """Ids of the entries that hold pattern within k edits, ascending: Sellers over every true entry."""
        pattern = bytes(pattern)
        if (pattern, k) not in self._ids:
            assert 0 <= k <= 3 and len(pattern) > k
            ids = [] if b'\n' in pattern else [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true)
                                               for line, e in enumerate(entries) if self.distance(e, pattern) <= k]
            self._ids[pattern, k] = np.array(ids, dtype=np.uint64)
        return self._ids[pattern, k]

    def ordered_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """The same ids in the order the engine states: chunk-major; inside a chunk by the piece index j of each entry's
        KEPT candidate (d, j), and inside one piece by the suffix that starts at d, text[d:] -- suffix-array order is the
        order of those suffixes as byte strings."""
        pattern = bytes(pattern)
        if (pattern, k) not in self._ordered:
            out = []
            for ch, entries in zip(self.chunks, self._true):
                keyed, start = [], 0
                for line, e in enumerate(entries):
                    if b'\n' not in pattern and self.distance(e, pattern) <= k:
                        d, j = kept_candidate(ch.text, pattern, k, start, start + len(e))
                        keyed.append((j, ch.text[d:], (ch.index << 32) | line))
                    start += len(e) + 1
                out += [i for _, _, i in sorted(keyed)]
            self._ordered[pattern, k] = np.array(out, dtype=np.uint64)
        return self._ordered[pattern, k]

    def piece_hits(self, pattern: bytes, k: int) -> int:
        """Exact occurrences of the pattern's pieces over every chunk, overlaps and repeated pieces counted: the
        candidates.  A pattern that holds a newline is not looked up at all."""
        pattern = bytes(pattern)
        if b'\n' in pattern:
            return 0
        return sum(int(occurrences(ch.text, piece).size) for ch in self.chunks for _, piece in pieces(pattern, k))
