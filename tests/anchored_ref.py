"""Brute-force reference of the anchored search (include/pss.h, "Anchored search"), in the style of tests/entry_id_ref.py:
no suffix array, no rewritten query.

The entries of a chunk are those of the entry ids: entry `line` starts at offset 0 (line 0) or at the byte after the
line-th 0x0A and ends before the next 0x0A, or at the end n of the text when none follows; a chunk has
count(0x0A) + (1 if n and text[n-1] != 0x0A) entries, empty ones included.  With s the start of an entry and e the
position of its closing newline (or n), a pattern of m bytes matches under
    START (1)        text[s:s+m] == pat and s + m <= e
    END (2)          text[e-m:e] == pat and e - m >= s
    START | END (3)  e - s == m and text[s:e] == pat
-- the three conditions are applied to every entry as they stand.  The text of a matching entry is the engine's for any
hit in it (IdChunk.entry: an unterminated last entry loses its last byte); the ids are not affected by that.
CPU only; tests/test_anchored_gpu.py compares every query of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdChunk, IdRef

START, END, ENTRY = 1, 2, 3
ANCHOR_OF = {'start': START, 'end': END, 'entry': ENTRY}


class AnchoredChunk(IdChunk):
    def __init__(self, text: bytes, index: int):
        super().__init__(text, index)
        n = len(text)
        k = self.num_entries
        nl = self.nl.tolist()
        self.starts = ([0] + [p + 1 for p in nl])[:k]
        self.ends = (nl + [n])[:k]

    def lines(self, pat: bytes, anchor: int) -> typing.List[int]:
        """Numbers of the entries of this chunk that pat matches under anchor, ascending."""
        assert anchor in (START, END, ENTRY)
        t, m = self.text, len(pat)
        out = []
        for line, (s, e) in enumerate(zip(self.starts, self.ends)):
            if anchor == START:
                ok = s + m <= e and t[s:s + m] == pat
            elif anchor == END:
                ok = e - m >= s and t[e - m:e] == pat
            else:
                ok = e - s == m and t[s:e] == pat
            if ok:
                out.append(line)
        return out

    def ids(self, pat: bytes, anchor: int) -> np.ndarray:       # (IdChunk.ids is the unanchored search: not used here)
        line = np.asarray(self.lines(pat, anchor), dtype=np.uint64)
        return (np.uint64(self.index) << np.uint64(32)) | line


class AnchoredRef(IdRef):
    """IdRef over AnchoredChunk: the same chunks, shards and entry texts; search_ids takes the anchor as well."""
    chunk_cls = AnchoredChunk

    def search_ids(self, pat: bytes, anchor: typing.Union[int, str]) -> np.ndarray:
        """Ids of the entries pat matches under anchor over every chunk, ascending."""
        anchor = ANCHOR_OF.get(anchor, anchor)
        parts = [ch.ids(pat, anchor) for ch in self.chunks]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)

    def entry(self, entry_id: int) -> bytes:
        by_index = {ch.index: ch for ch in self.chunks}
        return by_index[int(entry_id) >> 32].entry(int(entry_id) & 0xffffffff)

    def num_entries(self) -> int:
        return sum(ch.num_entries for ch in self.chunks)
