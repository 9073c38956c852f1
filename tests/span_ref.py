"""Brute-force reference of the match spans (include/pss.h, pss_reader_match_spans), on top of the entry-id reference of
tests/entry_id_ref.py: no pieces, no band and no suffix array.

Over an entry's TRUE bytes e (tests/glob_ref.true_entries) every candidate e[s : s + l] is enumerated -- l = len(p) and the
distance a byte-by-byte mismatch count, or with `edits` l = max(1, L - k) .. L + k and the distance a full, unbanded
Levenshtein table -- both sides folded first under `icase`, and the answer is the min of (d, s, -l) over the candidates
with d <= k: (start, length, distance), or (-1, 0, -1) where there is none or the pattern holds a newline.

span_naive is that sentence word for word, one table per candidate.  span computes the same over all starts at once (one
full table per start, whose last column holds every length's distance; numpy over the starts) and is what the suites
call; tests/test_span_ref.py holds the two against each other and against tests/edit_ref.sellers / tests/near_ref.
CPU only."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef
from tests.glob_ref import true_entries

NONE = (-1, 0, -1)
_MEMO = {}          # (entry, pattern, k, edits, icase) -> span: the suites of one run share the answers
_FOLD = bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))


def fold(b: bytes) -> bytes:
    """A-Z to a-z, nothing else."""
    return bytes(b).translate(_FOLD)


def lev(a: bytes, b: bytes) -> int:
    """Levenshtein distance over bytes: the full table, row by row."""
    row = list(range(len(b) + 1))
    for i, c in enumerate(a, 1):
        new = [i]
        for j, d in enumerate(b, 1):
            new.append(min(row[j - 1] + (c != d), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[-1]


def span_naive(entry: bytes, pattern: bytes, k: int, edits: bool = False, icase: bool = False) -> typing.Tuple[int, int, int]:
    """(start, length, distance) by the contract's own words: every (s, l), one distance each, the min of (d, s, -l)."""
    if b'\n' in pattern:
        return NONE
    e, p = (fold(entry), fold(pattern)) if icase else (bytes(entry), bytes(pattern))
    L = len(p)
    assert 0 <= k <= 3 and L > k
    best = None
    for l in (range(max(1, L - k), L + k + 1) if edits else (L,)):
        for s in range(len(e) - l + 1):
            w = e[s:s + l]
            d = lev(w, p) if edits else sum(x != y for x, y in zip(w, p))
            if d <= k and (best is None or (d, s, -l) < best):
                best = (d, s, -l)
    return NONE if best is None else (best[1], -best[2], best[0])


def _distances(e: np.ndarray, p: np.ndarray, lengths: typing.Sequence[int]) -> np.ndarray:
    """dist[s, j] = lev(e[s : s + lengths[j]], p) for every start s: per start the full table of e[s:] against p, row x
    = the x bytes taken, whose last column is read at the asked lengths.  Bytes past the entry's end equal nothing; the
    caller drops the candidates that reach there."""
    E, L, W = len(e), len(p), max(lengths)
    pad = np.full(E + W, 256, dtype=np.int16)
    pad[:E] = e
    win = np.lib.stride_tricks.sliding_window_view(pad, W)[:E]
    prev = np.tile(np.arange(L + 1, dtype=np.int64), (E, 1))           # no byte taken: lev('', p[:i]) = i
    last = np.empty((E, W + 1), dtype=np.int64)
    last[:, 0] = L
    cols = np.arange(L + 1, dtype=np.int64)[None, :]
    for x in range(1, W + 1):
        neq = win[:, x - 1, None] != p[None, :]
        cand = np.minimum(prev[:, :-1] + neq, prev[:, 1:] + 1)       # substitute or match, delete the text byte
        # ... or insert the pattern byte: new[i] = min(cand[i], new[i - 1] + 1) = the least cand[j] + (i - j) over j <= i
        head = np.concatenate([np.full((E, 1), x, dtype=np.int64), cand], axis=1) - cols
        new = np.minimum.accumulate(head, axis=1) + cols
        last[:, x] = new[:, L]
        prev = new
    return last[:, list(lengths)]


def candidates(entry: bytes, pattern: bytes, k: int, edits: bool = False, icase: bool = False) -> np.ndarray:
    """Every candidate within k as a row (d, s, l), int64 [m, 3], sorted by (d, s, -l): row 0 is the answer."""
    none = np.zeros((0, 3), dtype=np.int64)
    if b'\n' in pattern:
        return none
    eb, pb = (fold(entry), fold(pattern)) if icase else (bytes(entry), bytes(pattern))
    e, p = np.frombuffer(eb, np.uint8), np.frombuffer(pb, np.uint8)
    E, L = len(e), len(p)
    assert 0 <= k <= 3 and L > k
    if E == 0:
        return none
    if edits:
        lengths = list(range(max(1, L - k), L + k + 1))
        d = _distances(e, p, lengths)
    else:
        lengths = [L]
        d = np.full((E, 1), L + 1, dtype=np.int64)
        if E >= L:
            d[:E - L + 1, 0] = (np.lib.stride_tricks.sliding_window_view(e, L) != p).sum(axis=1)
    ls = np.array(lengths, dtype=np.int64)
    s = np.arange(E, dtype=np.int64)[:, None]
    at = np.nonzero((d <= k) & (s + ls[None, :] <= E))
    rows = np.stack([d[at], at[0], ls[at[1]]], axis=1)
    return rows[np.lexsort((-rows[:, 2], rows[:, 1], rows[:, 0]))]


def span(entry: bytes, pattern: bytes, k: int, edits: bool = False, icase: bool = False) -> typing.Tuple[int, int, int]:
    """(start, length, distance): span_naive's answer, all starts at once."""
    c = candidates(entry, pattern, k, edits, icase)
    return (int(c[0, 1]), int(c[0, 2]), int(c[0, 0])) if len(c) else NONE


class SpanRef(IdRef):
    """The chunks a reader holds, every entry with its true bytes."""

    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = {ch.index: true_entries(ch.text, ch.nl) for ch in self.chunks}
        assert all(len(self._true[ch.index]) == ch.num_entries for ch in self.chunks)

    def all_ids(self) -> np.ndarray:
        """Every entry id of the reference, chunk-major."""
        return np.array([(ch.index << 32) | line for ch in self.chunks for line in range(ch.num_entries)], dtype=np.uint64)

    def true_entry(self, entry_id: int) -> bytes:
        return self._true[int(entry_id) >> 32][int(entry_id) & 0xffffffff]

    def span(self, entry_id: int, pattern: bytes, k: int, edits: bool = False, icase: bool = False):
        key = (self.true_entry(entry_id), bytes(pattern), k, edits, icase)
        if key not in _MEMO:
            _MEMO[key] = span(*key)
        return _MEMO[key]

    def spans(self, ids, counts, patterns, budgets, edits: bool = False, icase: bool = False) -> np.ndarray:
        """What Reader.match_spans_batch(ids, counts, patterns, budgets, edits, icase=icase) returns: int32 [len(ids), 3]."""
        budgets = [budgets] * len(patterns) if isinstance(budgets, int) else list(budgets)
        ids = [int(i) for i in np.asarray(ids, dtype=np.uint64).tolist()]
        assert sum(int(c) for c in counts) == len(ids) and len(counts) == len(patterns) == len(budgets)
        out, pos = np.empty((len(ids), 3), dtype=np.int32), 0
        for c, p, k in zip(counts, patterns, budgets):
            for i in range(pos, pos + int(c)):
                out[i] = self.span(ids[i], p, k, edits, icase)
            pos += int(c)
        return out
