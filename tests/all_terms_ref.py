"""Brute-force reference of the all-terms search (include/pss.h, pss_reader_search_terms_batch), on top of the entry-id
reference of tests/entry_id_ref.py: no suffix array, no driver term, no verify step.

A group is (include terms, exclude terms).  Its answer is

    intersection of IdRef.search_ids(t) over the include terms  minus  union of IdRef.search_ids(t) over the exclude terms

so "an entry contains a term" means exactly what the plain search means (bytes.find over the chunk's text, the entry
start of every occurrence).  A term that holds a newline occurs in no ENTRY -- bytes.find may still find it across two
entries -- so the reference takes it out by the rule the contract states: as an include term it empties the group, as an
exclude term it excludes nothing.  CPU only; tests/test_all_terms_gpu.py compares every group of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef

EMPTY = np.zeros(0, dtype=np.uint64)


def split_group(group) -> typing.Tuple[typing.List[bytes], typing.List[bytes]]:
    """(include, exclude) of a group as Reader.search_all_ids_batch takes it: a pair of sequences, or a bare sequence of
    byte strings (no exclusions)."""
    group = list(group)
    if len(group) == 2 and not isinstance(group[0], bytes) and not isinstance(group[1], bytes):
        return list(group[0]), list(group[1])
    return group, []


class AllTermsRef(IdRef):
    def term_ids(self, term: bytes) -> np.ndarray:
        """Ids of the entries that hold term (ascending); none for a term with a newline."""
        assert term, 'an empty term is an argument error, not a search'
        return EMPTY if b'\n' in term else self.search_ids(term)

    def search_all_ids(self, group) -> np.ndarray:
        """Ids of the entries that hold every include term and no exclude term of the group, ascending."""
        include, exclude = split_group(group)
        assert include, 'a group without an include term is an argument error, not a search'
        ids = self.term_ids(include[0])
        for t in include[1:]:
            ids = np.intersect1d(ids, self.term_ids(t))
        for t in exclude:
            ids = np.setdiff1d(ids, self.term_ids(t))
        return ids.astype(np.uint64)
