"""Brute-force reference of the regular-expression search (include/pss.h, pss_reader_search_regex_batch), on top of the
wildcard reference of tests/glob_ref.py: no suffix array, no DFA.

The answer is Python's own: re.search(pattern, entry, re.I if fold else 0) over every entry's TRUE bytes (an unterminated
last entry keeps its last byte).  A pattern one of whose required literals holds a newline matches nothing.
What the engine states beyond the answer is restated too: per (pattern, chunk) pair the DRIVER is the rarest required
literal (regex_literals; occurrences counted in the chunk's text, overlapping ones included -- under fold the folded
occurrences of the literal's seed, as in tests/glob_class_ref.py), the lowest index on a tie; a chunk that lacks a literal
counts 0; `hits` is the sum of the drivers' counts.  CPU only."""
import re
import typing

import numpy as np

from tests import search_harness as H
from tests.glob_class_ref import occurrences
from tests.glob_ref import GlobRef
from tests.icase_ref import folded_occurrences

EMPTY = np.zeros(0, dtype=np.uint64)


def as_bytes(pattern) -> bytes:
    return pattern.encode('utf-8') if isinstance(pattern, str) else bytes(pattern)


class RegexRef(GlobRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._occ: typing.Dict[typing.Tuple[int, bytes, bool], int] = {}

    # ---- the answer ----
    def search_regex_ids(self, pattern, fold: bool = False) -> np.ndarray:
        """Ids of the entries the pattern matches, ascending."""
        from pysubstringsearch_amd import regex_literals
        pattern = as_bytes(pattern)
        if any(b'\n' in lit for lit in regex_literals(pattern, fold)):
            return EMPTY
        rx = re.compile(pattern, re.I if fold else 0)
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true) for line, e in enumerate(entries) if rx.search(e)]
        return np.array(ids, dtype=np.uint64)

    # ---- the driver and the hits ----
    def literal_hits(self, c: int, lit: bytes, fold: bool) -> int:
        key = (c, lit, fold)
        if key not in self._occ:
            text = self.chunks[c].text
            if not text:
                self._occ[key] = 0
            elif fold:
                from pysubstringsearch_amd import icase_variants
                self._occ[key] = folded_occurrences(text, icase_variants(lit)[1][0].lower())
            else:
                self._occ[key] = occurrences(text, lit)
        return self._occ[key]

    def driver(self, c: int, pattern, fold: bool = False) -> typing.Tuple[typing.Optional[int], int]:
        """(index of the driving literal among regex_literals(pattern), or None; the pair's hits) in chunk c."""
        from pysubstringsearch_amd import regex_literals
        lits = regex_literals(as_bytes(pattern), fold)
        if any(b'\n' in lit for lit in lits):
            return None, 0
        hits = [self.literal_hits(c, lit, fold) for lit in lits]
        best = min(hits)
        return (hits.index(best), best) if best else (None, 0)

    def hits(self, batch, fold: bool = False) -> int:
        return sum(self.driver(c, p, fold)[1] for p in batch for c in range(len(self.chunks)))


def _kind(fold):
    return H.Kind('regex_icase' if fold else 'regex', RegexRef,
                  ids=lambda r, b: r.search_regex_ids_batch(b, icase=fold),
                  packed=lambda r, b: r.search_regex_batch_packed(b, icase=fold),
                  counts=lambda r, b: r.count_regex_bytes(b, icase=fold),
                  rows=H._listed, want=lambda ref, p: ref.search_regex_ids(p, fold),
                  want_hits=lambda ref, b: ref.hits(b, fold))


REGEX, REGEX_ICASE = _kind(False), _kind(True)
