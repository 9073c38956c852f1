"""Brute-force reference of the case-insensitive all-terms and wildcard search (include/pss.h,
pss_reader_search_terms_icase_batch / pss_reader_search_seq_icase_batch), on top of the entry-id reference of
tests/entry_id_ref.py: no suffix array, no spellings, no verify step.

Per chunk every entry's TRUE bytes are enumerated (tests/glob_ref.true_entries).  bytes.lower folds A .. Z alone, which is
exactly the contract, so
  all-terms:  all(t.lower() in e.lower() for the include terms) and no exclude term so; an include term with a newline
              empties the group, an exclude term with one excludes nothing;
  glob:       glob_ref.glob_regex over the lower-cased segments, full-matched against the lower-cased entry.
What the engine states beyond the answer is computed too, from the expansion pss_icase_variants shows: per (group, chunk)
pair the DRIVER -- the include term (segment) whose seed has the fewest folded occurrences in the chunk's text, the
lowest index on a tie --, the `hits` of a batch (the sum of the drivers' seed occurrences; a pair with a void include
term has none) and the order inside a pair: by the suffix that starts at the driver's seed inside each entry's LEFTMOST
folded match of the driver term.  CPU only; tests/test_icase_groups_gpu.py compares every group of every case."""
import typing

import numpy as np

from tests.all_terms_ref import split_group
from tests.entry_id_ref import IdRef
from tests.glob_ref import glob_regex, true_entries
from tests.icase_ref import folded_occurrences

EMPTY = np.zeros(0, dtype=np.uint64)


def seed_of(term: bytes) -> typing.Tuple[int, bytes]:
    """(seed_off, seed) of a term under the configured PSS_ICASE_SEED_LETTERS."""
    from pysubstringsearch_amd import icase_variants
    off, var = icase_variants(bytes(term))
    return off, var[0]


def holds_all(entry: bytes, group) -> bool:
    """Does the entry (true bytes) match the all-terms group under fold?"""
    include, exclude = split_group(group)
    assert include and all(include) and all(exclude)
    if any(b'\n' in t for t in include):
        return False
    e = bytes(entry).lower()
    return all(bytes(t).lower() in e for t in include) and not any(bytes(t).lower() in e for t in exclude if b'\n' not in t)


def matches_seq(entry: bytes, segments: typing.Sequence[bytes], anchors: int) -> bool:
    """Does the entry (true bytes) match (segments, anchors) under fold?"""
    if any(b'\n' in s for s in segments):
        return False
    return glob_regex([bytes(s).lower() for s in segments], anchors).fullmatch(bytes(entry).lower()) is not None


def matches_glob(entry: bytes, pattern: bytes) -> bool:
    from pysubstringsearch_amd import glob_parse
    return matches_seq(entry, *glob_parse(pattern))


class IcaseGroupsRef(IdRef):
    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = [true_entries(ch.text, ch.nl) for ch in self.chunks]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._true, self.chunks))
        self._occ: typing.Dict[typing.Tuple[int, bytes], int] = {}

    # ---- the answer ----
    def _ids(self, keep) -> np.ndarray:
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._true) for line, e in enumerate(entries) if keep(e)]
        return np.array(ids, dtype=np.uint64)

    def search_all_ids(self, group) -> np.ndarray:
        """Ids of the entries that match the all-terms group under fold, ascending."""
        return self._ids(lambda e: holds_all(e, group))

    def search_seq_ids(self, segments, anchors: int) -> np.ndarray:
        return self._ids(lambda e: matches_seq(e, segments, anchors))

    def search_glob_ids(self, pattern: bytes) -> np.ndarray:
        """Ids of the entries that match the glob pattern under fold, ascending."""
        from pysubstringsearch_amd import glob_parse
        return self.search_seq_ids(*glob_parse(pattern))

    # ---- the driver, the hits, the order ----
    def seed_hits(self, c: int, term: bytes) -> int:
        """Folded occurrences of term's seed in chunk c (position in self.chunks)."""
        seed = seed_of(term)[1].lower()
        key = (c, seed)
        if key not in self._occ:
            self._occ[key] = folded_occurrences(self.chunks[c].text, seed) if self.chunks[c].text else 0
        return self._occ[key]

    def driver(self, c: int, include: typing.Sequence[bytes]) -> typing.Tuple[typing.Optional[int], int]:
        """(index of the driver among the include terms or None for a pair without hits, the pair's hits) in chunk c."""
        if any(b'\n' in t for t in include):
            return None, 0
        hits = [self.seed_hits(c, t) for t in include]
        best = min(hits)
        return (hits.index(best), best) if best else (None, 0)

    def _include(self, kind: str, q) -> typing.List[bytes]:
        if kind == 'all':
            return [bytes(t) for t in split_group(q)[0]]
        from pysubstringsearch_amd import glob_parse
        return [bytes(s) for s in glob_parse(q)[0]]

    def hits(self, kind: str, batch) -> int:
        """The `hits` of a batch: the drivers' seed occurrences over every (group, chunk) pair."""
        return sum(self.driver(c, self._include(kind, q))[1] for q in batch for c in range(len(self.chunks)))

    def drivers(self, kind: str, q) -> typing.List[typing.Optional[int]]:
        """The driver's index among the include terms (segments) of q, per chunk."""
        return [self.driver(c, self._include(kind, q))[0] for c in range(len(self.chunks))]

    def ordered_ids(self, kind: str, q) -> np.ndarray:
        """The ids of q in the order the engine states: chunk-major, and inside a chunk by the suffix that starts at the
        driver term's seed (seed_off bytes into the match) inside each entry's leftmost folded match of the driver term."""
        include = self._include(kind, q)
        keep = (lambda e: holds_all(e, q)) if kind == 'all' else (lambda e: matches_glob(e, q))
        out: typing.List[int] = []
        for c, (ch, entries) in enumerate(zip(self.chunks, self._true)):
            d, _ = self.driver(c, include)
            if d is None:
                assert not any(keep(e) for e in entries)
                continue
            low, so = include[d].lower(), seed_of(include[d])[0]
            keyed, start = [], 0
            for line, e in enumerate(entries):
                if keep(e):
                    at = e.lower().find(low)
                    assert at >= 0
                    keyed.append((ch.text[start + at + so:], (ch.index << 32) | line))
                start += len(e) + 1
            out += [i for _, i in sorted(keyed)]
        return np.array(out, dtype=np.uint64)
