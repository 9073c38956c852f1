"""Brute-force restatement of Reader::search (reference src/lib.rs:201-287) that uses no suffix array.

For one query over one chunk text: every occurrence, overlapping ones included, by repeated bytes.find (the
empty query occurs at every position 0 .. n-1); the entry of a hit at di runs from the byte after the last
'\\n' before di to the first '\\n' at or after di, or to dlen - 1 when none follows (lib.rs:266-273, as
oracle/pss_oracle.c restates it); one entry per (query, chunk, entry start).  The chunk texts come from the
container itself (OracleReader(path).chunk(c)[0]), so the Writer's chunking rule is not restated here.
CPU only; tests/test_search_edges_gpu.py compares every search route of the engine with it."""
import typing

import numpy as np


def occurrences(text: bytes, query: bytes) -> np.ndarray:
    """Start of every occurrence of query in text, overlapping ones included, ascending."""
    n = len(text)
    if not query:
        return np.arange(n, dtype=np.int64)
    out = []
    i = text.find(query)
    while i >= 0:
        out.append(i)
        i = text.find(query, i + 1)
    return np.asarray(out, dtype=np.int64)


class Chunk:
    """One chunk text with its newline positions (the entry bounds of many hits at once)."""

    def __init__(self, text: bytes):
        self.text = text
        self.nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 0x0A).astype(np.int64)

    def entries(self, query: bytes) -> typing.List[bytes]:
        """The entries of query in this chunk, one per distinct entry start, in text order."""
        hits = occurrences(self.text, query)
        if hits.size == 0:
            return []
        n = len(self.text)
        # last '\n' before di -> start; first '\n' at or after di -> end (no newline: n - 1)
        k = np.searchsorted(self.nl, hits, side='left')          # newlines before di: nl[:k]
        start = np.zeros_like(hits)
        before = k > 0
        start[before] = self.nl[k[before] - 1] + 1
        end = np.full_like(hits, n - 1)
        after = k < self.nl.size
        end[after] = self.nl[k[after]]
        _, first = np.unique(start, return_index=True)
        return [self.text[int(start[i]):int(end[i])] for i in sorted(first)]


class SearchRef:
    """The reference result of a whole index: per query, the multiset of its entries over every chunk."""

    def __init__(self, texts: typing.Sequence[bytes]):
        self.chunks = [Chunk(t) for t in texts]

    @classmethod
    def from_index(cls, path: str) -> 'SearchRef':
        from oracle import oracle as O
        r = O.OracleReader(path)
        try:
            texts = [r.chunk(c)[0] for c in range(r.num_chunks)]
        finally:
            r.close()
        return cls(texts)

    def hits(self, query: bytes) -> typing.List[int]:
        """Occurrences of query in every chunk (the suffix-array hits of each (query, chunk) pair)."""
        return [int(occurrences(ch.text, query).size) for ch in self.chunks]

    def search(self, query: bytes) -> typing.List[bytes]:
        out = []
        for ch in self.chunks:
            out.extend(ch.entries(query))
        return out

    def search_multiple(self, queries: typing.Sequence[bytes]) -> typing.Tuple[typing.List[bytes], typing.List[int]]:
        """Entries query-major (chunk order inside a query) and the count of each query."""
        ents, counts = [], []
        for q in queries:
            e = self.search(q)
            ents.extend(e)
            counts.append(len(e))
        return ents, counts
