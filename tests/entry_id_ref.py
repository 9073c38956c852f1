"""Brute-force reference of the entry ids (include/pss.h, "Entry ids"), in the style of tests/search_ref.py: no suffix
array, no line table.

An entry id is (chunk index in the index file << 32) | line, line = the number of 0x0A bytes of the chunk's text before
the entry's first byte.  For one query over one chunk: every occurrence by repeated bytes.find (search_ref.occurrences),
the entry start of a hit = the byte after the last newline before it, line = searchsorted(newline positions, start,
'left'), one id per distinct start.  The text of an entry follows the engine's entry rule (search_ref.Chunk: to the next
newline, or to n - 1 when none follows).  CPU only; tests/test_entry_ids_gpu.py compares every query of every case."""
import typing

import numpy as np

from tests.search_ref import Chunk, occurrences


class IdChunk(Chunk):
    def __init__(self, text: bytes, index: int):
        super().__init__(text)
        self.index = index

    @property
    def num_entries(self) -> int:
        n = len(self.text)
        return int(self.nl.size) + (1 if n and self.text[-1] != 0x0A else 0)

    def ids(self, query: bytes) -> np.ndarray:
        """Ids of the entries of this chunk that hold query, ascending."""
        hits = occurrences(self.text, query)
        if hits.size == 0:
            return np.zeros(0, dtype=np.uint64)
        k = np.searchsorted(self.nl, hits, side='left')          # newlines before the hit
        start = np.zeros_like(hits)
        before = k > 0
        start[before] = self.nl[k[before] - 1] + 1
        start = np.unique(start)
        line = np.searchsorted(self.nl, start, side='left').astype(np.uint64)
        return (np.uint64(self.index) << np.uint64(32)) | line

    def entry(self, line: int) -> bytes:
        """Text of entry `line`."""
        assert 0 <= line < self.num_entries
        start = 0 if line == 0 else int(self.nl[line - 1]) + 1
        end = int(self.nl[line]) if line < self.nl.size else len(self.text) - 1
        return self.text[start:end]


class IdRef:
    """The chunks of one index (or the ones a shard holds: `indices` = their indexes in the file)."""
    chunk_cls = IdChunk             # (a reference of another kind of search names its own chunk class here)

    def __init__(self, texts: typing.Sequence[bytes], indices: typing.Optional[typing.Sequence[int]] = None):
        indices = list(range(len(texts))) if indices is None else list(indices)
        self.chunks = [self.chunk_cls(t, i) for t, i in zip(texts, indices)]

    @classmethod
    def from_index(cls, path: str, keep=lambda c: True) -> 'IdRef':
        """Chunk texts from the container itself; empty chunks keep their index and hold nothing."""
        from tests.search_ref import SearchRef
        texts = [ch.text for ch in SearchRef.from_index(path).chunks]
        held = [c for c in range(len(texts)) if keep(c)]
        return cls([texts[c] for c in held], held)

    def search_ids(self, query: bytes) -> np.ndarray:
        """Ids of query over every chunk, ascending (chunk-major, line order inside a chunk)."""
        parts = [ch.ids(query) for ch in self.chunks]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def entry_counts(self) -> typing.Dict[int, int]:
        return {ch.index: ch.num_entries for ch in self.chunks if len(ch.text)}

    def entry(self, entry_id: int) -> bytes:
        by_index = {ch.index: ch for ch in self.chunks}
        return by_index[int(entry_id) >> 32].entry(int(entry_id) & 0xffffffff)
