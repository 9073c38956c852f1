"""Brute-force reference of the wildcard search with byte classes (include/pss.h, pss_reader_search_seqc_batch), on top
of the wildcard reference of tests/glob_ref.py: no suffix array, no cores in the answer, no greedy walk.

(segments, anchors) in the form of glob_parse(pattern, classes=True) -- a segment is a list with one bytes object per
position, the bytes the position accepts -- become one bytes regular expression under fullmatch over every entry's TRUE
bytes: each position an explicit set of escaped bytes, [^\\n]* for `*`.  A literal newline matches nothing.  Under fold
the reference closes the sets ITSELF, from the pattern's text: it finds out with a scan of its own which positions were
written negated, adds the other case of every letter to a set written plain and takes both cases of a letter out of a
set written negated unless it holds both; a literal accepts both of its cases.
What the engine states beyond the answer is restated too: per (pattern, chunk) pair the DRIVER is the rarest core
(glob_cores: the longest literal run of a segment, the leftmost on a tie; occurrences counted in the chunk's text, under
fold the folded occurrences of the core's seed), the lowest index on a tie; a chunk that lacks a core counts 0; `hits` is
the sum of the drivers' counts.  CPU only."""
import re
import typing

import numpy as np

from tests.glob_ref import ANY, END, START, GlobRef
from tests.icase_ref import folded_occurrences

EMPTY = np.zeros(0, dtype=np.uint64)


def _byte(b: int) -> bytes:
    return b'\\x%02x' % b


def position_regex(members: bytes) -> bytes:
    assert members
    return b'[' + b''.join(_byte(b) for b in members) + b']'


def class_regex(segments, anchors: int) -> 're.Pattern':
    assert segments and all(segments) and 0 <= anchors <= 3
    body = ANY.join(b''.join(position_regex(pos) for pos in seg) for seg in segments)
    return re.compile((b'' if anchors & START else ANY) + body + (b'' if anchors & END else ANY), re.DOTALL)


def swapcase(b: int) -> int:
    return b ^ 0x20 if 0x41 <= (b & 0xDF) <= 0x5A else b


def negated_positions(pattern: bytes) -> typing.List[typing.List[bool]]:
    """Per segment, per position of the pattern: was the position written as a negated set?  A scan of the reference's own
    (the pattern is well formed: glob_parse has accepted it)."""
    out, cur = [], []
    i, n = 0, len(pattern)
    while i < n:
        c = pattern[i:i + 1]
        if c == b'*':
            if cur:
                out.append(cur)
                cur = []
            i += 1
        elif c == b'\\':
            cur.append(False)
            i += 2
        elif c == b'[':
            neg = pattern[i + 1:i + 2] == b'!'
            j = i + (2 if neg else 1)
            if pattern[j:j + 1] == b']':
                j += 1
            while pattern[j:j + 1] != b']':
                j += 2 if pattern[j:j + 1] == b'\\' else 1
            cur.append(neg)
            i = j + 1
        else:
            cur.append(False)
            i += 1
    if cur:
        out.append(cur)
    return out


def fold_closed(segments, negated):
    """The segments as they match under fold."""
    out = []
    for seg, negs in zip(segments, negated):
        assert len(seg) == len(negs)
        row = []
        for pos, neg in zip(seg, negs):
            have = set(pos)
            if neg:
                have = {b for b in have if swapcase(b) in have}
            else:
                have |= {swapcase(b) for b in have}
            row.append(bytes(sorted(have)))
        out.append(row)
    return out


def occurrences(text: bytes, pat: bytes) -> int:
    """Occurrences of pat in text, overlapping ones included."""
    k, at = 0, text.find(pat)
    while at >= 0:
        k += 1
        at = text.find(pat, at + 1)
    return k


class GlobClassRef(GlobRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._occ: typing.Dict[typing.Tuple[int, bytes, bool], int] = {}

    # ---- the answer ----
    def search_class_ids(self, segments, anchors: int) -> np.ndarray:
        """Ids of the entries that match (segments, anchors), ascending."""
        if any(pos == b'\n' for seg in segments for pos in seg):
            return EMPTY
        rx = class_regex(segments, anchors)
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true) for line, e in enumerate(entries) if rx.fullmatch(e)]
        return np.array(ids, dtype=np.uint64)

    def parsed(self, pattern: bytes, fold: bool = False):
        from pysubstringsearch_amd import glob_parse
        segments, anchors = glob_parse(pattern, classes=True)
        if fold:
            segments = fold_closed(segments, negated_positions(pattern))
        return segments, anchors

    def search_glob_ids(self, pattern: bytes, fold: bool = False) -> np.ndarray:
        """The same for a glob pattern as Reader.search_glob_ids_batch(..., classes=True, icase=fold) takes it."""
        return self.search_class_ids(*self.parsed(pattern, fold))

    # ---- the driver and the hits ----
    def core_hits(self, c: int, core: bytes, fold: bool) -> int:
        key = (c, core, fold)
        if key not in self._occ:
            text = self.chunks[c].text
            if not text:
                self._occ[key] = 0
            elif fold:
                from pysubstringsearch_amd import icase_variants
                self._occ[key] = folded_occurrences(text, icase_variants(core)[1][0].lower())
            else:
                self._occ[key] = occurrences(text, core)
        return self._occ[key]

    def driver(self, c: int, pattern: bytes, fold: bool = False) -> typing.Tuple[typing.Optional[int], int]:
        """(index of the driving core among the pattern's cores, or None; the pair's hits) in chunk c."""
        from pysubstringsearch_amd import glob_cores, glob_parse
        if any(pos == b'\n' for seg in glob_parse(pattern, classes=True)[0] for pos in seg):
            return None, 0
        cores = [core[1] for core in glob_cores(pattern) if core is not None]
        hits = [self.core_hits(c, core, fold) for core in cores]
        best = min(hits)
        return (hits.index(best), best) if best else (None, 0)

    def hits(self, batch, fold: bool = False) -> int:
        return sum(self.driver(c, p, fold)[1] for p in batch for c in range(len(self.chunks)))
