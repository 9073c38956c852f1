"""Brute-force reference of the search within k mismatches (include/pss.h, pss_reader_search_near_batch), on top of the
entry-id reference of tests/entry_id_ref.py: no suffix array and no pieces in what decides a match.

Per chunk every entry's TRUE bytes are enumerated (tests/glob_ref.true_entries: text[start : newline], or text[start : n]
for an unterminated last entry) and an entry matches pattern p within k when ANY window of len(p) of those bytes differs
from p in at most k positions -- the windows of an entry never reach over its newline, because the entry's bytes hold
none.  A pattern that holds a newline matches nothing.  ordered_ids states the order contract and piece_hits what the
`hits` of a batch are pinned to; only those two know the pieces, restated here as pattern[j * L // (k + 1) : (j + 1) * L
// (k + 1)].  CPU only; tests/test_near_gpu.py compares every pattern of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef
from tests.glob_ref import true_entries
from tests.search_ref import occurrences


def pieces(pattern: bytes, k: int) -> typing.List[typing.Tuple[int, bytes]]:
    """[(offset, piece)] of a pattern of more than k bytes: the contract's cut, restated."""
    L = len(pattern)
    assert 0 <= k < L
    cut = [j * L // (k + 1) for j in range(k + 2)]
    return [(cut[j], pattern[cut[j]:cut[j + 1]]) for j in range(k + 1)]


def window_mismatches(entry: bytes, pattern: bytes) -> np.ndarray:
    """Mismatches of pattern against every window of its length in entry: one count per start 0 .. len(entry) - len(pattern)."""
    L = len(pattern)
    if len(entry) < L:
        return np.zeros(0, dtype=np.int64)
    e, p = np.frombuffer(entry, np.uint8), np.frombuffer(pattern, np.uint8)
    return (np.lib.stride_tricks.sliding_window_view(e, L) != p).sum(axis=1)


def near_starts(entry: bytes, pattern: bytes, k: int) -> np.ndarray:
    """Start of every window of entry within k mismatches of pattern, ascending."""
    return np.flatnonzero(window_mismatches(entry, pattern) <= k)


def rule_set_lines(text: bytes, pattern: bytes, k: int) -> typing.List[int]:
    """The lines of ONE chunk text that the engine's rule set keeps, in the engine's order -- the rules of DESIGN.md
    4.15 restated hit by hit, so that they can be held against the brute force above without a GPU: every exact
    occurrence di of every piece j, piece-major and in suffix order inside a piece, is a hit; with m = di - off_j it
    survives iff the window [m, m + L) lies in the chunk (1) and in di's entry (2, 3), differs from the pattern in at
    most k bytes (4), no piece j' < j is exact in it (5), and no window within budget starts in [entry start, m)."""
    if b'\n' in pattern:
        return []
    n, L = len(text), len(pattern)
    nl = [i for i, b in enumerate(text) if b == 0x0A]
    p = np.frombuffer(pattern, np.uint8)
    t = np.frombuffer(text, np.uint8)
    miss = lambda s: int((t[s:s + L] != p).sum())
    cut, kept = pieces(pattern, k), []
    for j, (off, piece) in enumerate(cut):
        for di in sorted(occurrences(text, piece).tolist(), key=lambda d: text[d:]):
            m = di - off
            if m < 0 or m + L > n:
                continue
            line = int(np.searchsorted(nl, di, side='left'))
            start = nl[line - 1] + 1 if line else 0
            end = nl[line] if line < len(nl) else n
            if m < start or m + L > end or miss(m) > k:
                continue
            if any(text[m + o:m + o + len(q)] == q for o, q in cut[:j]):
                continue
            if any(miss(s) <= k for s in range(start, m)):
                continue
            kept.append(line)
    return kept


class NearRef(IdRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = [true_entries(ch.text, ch.nl) for ch in self.chunks]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._true, self.chunks))
        self._ids, self._ordered = {}, {}       # (computed once per (pattern, k): the tests of one index share them)

    def search_near_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """Ids of the entries that hold pattern within k mismatches, ascending."""
        pattern = bytes(pattern)
        if (pattern, k) not in self._ids:
            self._ids[pattern, k] = self._search_near_ids(pattern, k)
        return self._ids[pattern, k]

    def ordered_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """The same ids in the order the engine states (below)."""
        pattern = bytes(pattern)
        if (pattern, k) not in self._ordered:
            self._ordered[pattern, k] = self._ordered_ids(pattern, k)
        return self._ordered[pattern, k]

    def _search_near_ids(self, pattern: bytes, k: int) -> np.ndarray:
        assert 0 <= k <= 3 and len(pattern) > k
        if b'\n' in pattern:
            return np.zeros(0, dtype=np.uint64)
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true) for line, e in enumerate(entries)
               if len(e) >= len(pattern) and near_starts(e, pattern, k).size]
        return np.array(ids, dtype=np.uint64)

    def _ordered_ids(self, pattern: bytes, k: int) -> np.ndarray:
        """The ids in the order the engine states: chunk-major; inside a chunk by the index j of the FIRST EXACT
        PIECE of each entry's LEFTMOST near match m, and inside one piece by the suffix that starts at that piece's
        occurrence, text[m + off_j:] -- suffix-array order is the order of those suffixes as byte strings."""
        if b'\n' in pattern:
            return np.zeros(0, dtype=np.uint64)
        cut, out = pieces(pattern, k), []
        for ch, entries in zip(self.chunks, self._true):
            keyed, start = [], 0
            for line, e in enumerate(entries):
                at = near_starts(e, pattern, k) if len(e) >= len(pattern) else ()
                if len(at):
                    m = int(at[0])
                    j, off = next((j, off) for j, (off, piece) in enumerate(cut) if e[m + off:m + off + len(piece)] == piece)
                    keyed.append((j, ch.text[start + m + off:], (ch.index << 32) | line))
                start += len(e) + 1
            out += [i for _, _, i in sorted(keyed)]
        return np.array(out, dtype=np.uint64)

    def piece_hits(self, pattern: bytes, k: int) -> int:
        """Exact occurrences of the pattern's pieces over every chunk, overlaps and repeated pieces counted: the
        candidates.  A pattern that holds a newline is not looked up at all."""
        pattern = bytes(pattern)
        if b'\n' in pattern:
            return 0
        return sum(int(occurrences(ch.text, piece).size) for ch in self.chunks for _, piece in pieces(pattern, k))
