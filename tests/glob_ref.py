"""Brute-force reference of the wildcard search (include/pss.h, pss_reader_search_seq_batch), on top of the entry-id
reference of tests/entry_id_ref.py: no suffix array, no driver segment, no greedy walk.

Per chunk every entry's TRUE bytes are enumerated -- text[start : newline], or text[start : n] for an unterminated last
entry: not IdChunk.entry, which drops that entry's last byte as the engine's text does -- and (segments, anchors) become
one bytes regular expression under fullmatch: re.escape of every segment joined by [^\\n]*, with [^\\n]* at an unanchored
end.  A segment that holds a newline matches nothing.  CPU only; tests/test_glob_gpu.py compares every pattern of every
case."""
import re
import typing

import numpy as np

from tests.entry_id_ref import IdRef

START, END = 1, 2
ANY = rb'[^\n]*'


def glob_regex(segments: typing.Sequence[bytes], anchors: int) -> 're.Pattern':
    assert segments and all(segments) and 0 <= anchors <= 3
    body = ANY.join(re.escape(bytes(s)) for s in segments)
    return re.compile((b'' if anchors & START else ANY) + body + (b'' if anchors & END else ANY), re.DOTALL)


def true_entries(text: bytes, nl: np.ndarray) -> typing.List[bytes]:
    """Every entry of a chunk with all its bytes, in line order."""
    out, start = [], 0
    for e in nl.tolist():
        out.append(text[start:e])
        start = e + 1
    if start < len(text):
        out.append(text[start:])             # no closing newline: up to n, the last byte included
    return out


class GlobRef(IdRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = [true_entries(ch.text, ch.nl) for ch in self.chunks]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._true, self.chunks))

    def search_seq_ids(self, segments: typing.Sequence[bytes], anchors: int) -> np.ndarray:
        """Ids of the entries that match (segments, anchors), ascending."""
        if any(b'\n' in s for s in segments):
            return np.zeros(0, dtype=np.uint64)
        rx = glob_regex(segments, anchors)
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true) for line, e in enumerate(entries) if rx.fullmatch(e)]
        return np.array(ids, dtype=np.uint64)

    def search_glob_ids(self, pattern: bytes) -> np.ndarray:
        """The same for a glob pattern as Reader.search_glob_ids_batch takes it."""
        from pysubstringsearch_amd import glob_parse
        return self.search_seq_ids(*glob_parse(pattern))
