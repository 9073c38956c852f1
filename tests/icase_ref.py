"""Brute-force reference of the case-insensitive search (include/pss.h, pss_reader_search_icase_batch), on top of the
entry-id reference of tests/entry_id_ref.py: no suffix array, no seed, no spellings.

Per chunk every entry's TRUE bytes are enumerated (tests/glob_ref.true_entries: text[start : newline], or text[start : n]
for an unterminated last entry) and an entry matches when p.lower() in e.lower() -- bytes.lower folds A .. Z alone, which
is exactly the contract.  A pattern that holds a newline matches nothing.  folded_occurrences counts what the `hits` of
a batch are pinned to: the occurrences of a byte string in a text under fold, overlapping ones included.  CPU only;
tests/test_icase_gpu.py compares every pattern of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef
from tests.glob_ref import true_entries


def folded_occurrences(text: bytes, piece: bytes) -> int:
    """Start positions of piece in text under ASCII case folding (overlaps count)."""
    text, piece = bytes(text).lower(), bytes(piece).lower()
    assert piece
    count, at = 0, text.find(piece)
    while at >= 0:
        count += 1
        at = text.find(piece, at + 1)
    return count


class IcaseRef(IdRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._low = [[e.lower() for e in true_entries(ch.text, ch.nl)] for ch in self.chunks]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._low, self.chunks))

    def search_icase_ids(self, pattern: bytes) -> np.ndarray:
        """Ids of the entries that hold pattern under fold, ascending."""
        pattern = bytes(pattern)
        assert pattern
        if b'\n' in pattern:
            return np.zeros(0, dtype=np.uint64)
        low = pattern.lower()
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._low) for line, e in enumerate(entries) if low in e]
        return np.array(ids, dtype=np.uint64)

    def seed_hits(self, seed: bytes) -> int:
        """Folded occurrences of a seed over every chunk: the candidates of its pattern."""
        return sum(folded_occurrences(ch.text, seed) for ch in self.chunks)

    def ordered_ids(self, pattern: bytes, seed_off: int) -> np.ndarray:
        """The same ids in the order the engine states: chunk-major, and inside a chunk by the suffix that starts at the
        seed's occurrence (seed_off bytes into the match) inside each entry's LEFTMOST folded match -- suffix-array
        order is the order of those suffixes as byte strings."""
        pattern = bytes(pattern)
        if b'\n' in pattern:
            return np.zeros(0, dtype=np.uint64)
        low, out = pattern.lower(), []
        for ch, entries in zip(self.chunks, self._low):
            keyed, start = [], 0
            for line, e in enumerate(entries):
                at = e.find(low)
                if at >= 0:
                    keyed.append((ch.text[start + at + seed_off:], (ch.index << 32) | line))
                start += len(e) + 1
            out += [i for _, i in sorted(keyed)]
        return np.array(out, dtype=np.uint64)
