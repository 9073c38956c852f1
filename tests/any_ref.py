"""Brute-force reference of the any-of search (include/pss.h, pss_reader_search_any_batch), on top of the entry-id reference
of tests/entry_id_ref.py: no suffix array, no seed, no normalisation in the answer itself.

Per chunk every entry's TRUE bytes are enumerated (tests/glob_ref.true_entries: text[start : newline], or text[start : n]
for an unterminated last entry) and an entry matches a set when any of the set's alternatives, AS GIVEN, is in it -- under
fold both sides through bytes.lower, which folds A .. Z alone.  An alternative that holds a newline is in no entry by that
very test.  Beside the answer the module restates what the engine documents about HOW it asks: the normalisation
(normalise), the seed rule (seed_letters, fold_seed, alternatives -- what any_alternatives must return), the order
(ordered_ids) and the `hits` of a batch.  ANY and ANY_ICASE are the search_harness.Kind objects of the two forms.  CPU
only; tests/test_any_gpu.py compares every set of every case."""
import typing

import numpy as np

from tests.entry_id_ref import IdRef
from tests.glob_ref import true_entries
from tests.icase_ref import folded_occurrences
from tests.search_harness import Kind, _listed
from tests.search_ref import occurrences

LETTERS = 5                     # the default of PSS_ICASE_SEED_LETTERS
MAX_ALTS, MAX_ALTS_ICASE = 64, 32


def normalise(alts: typing.Sequence[bytes], icase: bool = False) -> typing.List[bytes]:
    """The five steps: fold, drop duplicates, drop what holds a newline, drop what holds another alternative, sort."""
    alts = [bytes(a).lower() if icase else bytes(a) for a in alts]
    alts = [a for a in set(alts) if b'\n' not in a]
    return sorted(a for a in alts if not any(b != a and b in a for b in alts))


def seed_letters(n: int, letters: int = LETTERS) -> int:
    """min(letters, floor(log2(64 / n))): the set keeps at most 64 queries."""
    f = 0
    while (64 // n) >> (f + 1):
        f += 1
    return min(letters, f)


def is_letter(b: int) -> bool:
    return 0x61 <= (b | 0x20) <= 0x7a


def fold_seed(alt: bytes, f: int) -> typing.Tuple[int, int]:
    """(offset, length) of the longest window of alt with at most f ASCII letters, the leftmost on a tie -- by trying every
    window, longest first."""
    for n in range(len(alt), 0, -1):
        for at in range(len(alt) - n + 1):
            if sum(is_letter(b) for b in alt[at:at + n]) <= f:
                return at, n
    raise AssertionError('f >= 1: a window of one byte always fits')


def alternatives(alts: typing.Sequence[bytes], icase: bool = False, letters: int = LETTERS):
    """[(alternative, seed position, seed bytes)] of the normalised set: what any_alternatives returns."""
    norm = normalise(alts, icase)
    if not icase:
        return [(a, 0, a) for a in norm]
    f = seed_letters(len(norm), letters) if norm else letters
    out = []
    for a in norm:
        at, n = fold_seed(a, f)
        out.append((a, at, a[at:at + n]))
    return out


def spellings(seed: bytes) -> typing.List[bytes]:
    """Every spelling of seed, ascending bytewise."""
    out = [b'']
    for b in seed:
        out = [s + bytes([c]) for s in out for c in ((b & ~0x20, b | 0x20) if is_letter(b) else (b,))]
    return sorted(out)


class AnyRef(IdRef):
    icase = False
    letters = LETTERS           # (a test that sets PSS_ICASE_SEED_LETTERS says so here)

    def __init__(self, texts, indices=None):
        super().__init__(texts, indices)
        self._true = [true_entries(ch.text, ch.nl) for ch in self.chunks]
        self._low = [[e.lower() for e in entries] for entries in self._true]
        assert all(len(t) == ch.num_entries for t, ch in zip(self._true, self.chunks))

    def _entries(self):
        return self._low if self.icase else self._true

    def _fold(self, b: bytes) -> bytes:
        return bytes(b).lower() if self.icase else bytes(b)

    def search_any_ids(self, alts: typing.Sequence[bytes]) -> np.ndarray:
        """Ids of the entries that hold at least one alternative, ascending."""
        alts = [self._fold(a) for a in alts]
        assert alts and all(alts)
        ids = [(ch.index << 32) | line for ch, entries in zip(self.chunks, self._entries()) for line, e in enumerate(entries)
               if any(a in e for a in alts)]
        return np.array(ids, dtype=np.uint64)

    def holding(self, alts: typing.Sequence[bytes]) -> typing.List[typing.Set[bytes]]:
        """Per entry (every chunk, in order) the distinct alternatives it holds: what the fuzz conditions are judged by."""
        alts = [self._fold(a) for a in alts]
        return [{a for a in alts if a in e} for entries in self._entries() for e in entries]

    def ordered_ids(self, alts: typing.Sequence[bytes]) -> np.ndarray:
        """The same ids in the order the engine states: chunk-major; inside a chunk by the alternative (ascending, of the
        normalised set) that stands at the entry's LEFTMOST match, under fold then by the spelling of its seed there, then
        in suffix-array order -- the order, as byte strings, of the suffixes that start at the query's occurrence."""
        asked = alternatives(alts, self.icase, self.letters)
        out = []
        for ch, entries in zip(self.chunks, self._entries()):
            keyed, start = [], 0
            for line, e in enumerate(entries):
                found = [(e.find(a), j) for j, (a, _, _) in enumerate(asked) if a in e]
                if found:
                    at, j = min(found)
                    assert sum(f[0] == at for f in found) == 1          # prefix-free: one alternative stands there
                    _, pos, seed = asked[j]
                    where = start + at + pos
                    keyed.append((j, ch.text[where:where + len(seed)], ch.text[where:], (ch.index << 32) | line))
                start += len(e) + 1
            out += [i for _, _, _, i in sorted(keyed)]
        return np.array(out, dtype=np.uint64)

    def hits(self, batch) -> int:
        """`hits` of a batch: the exact occurrences of every query in every chunk -- the alternatives of the normalised
        sets, or under fold the folded occurrences of their seeds (every spelling is a query)."""
        total = 0
        for alts in batch:
            for _, _, seed in alternatives(alts, self.icase, self.letters):
                for ch in self.chunks:
                    total += folded_occurrences(ch.text, seed) if self.icase else int(occurrences(ch.text, seed).size)
        return total


class AnyIcaseRef(AnyRef):
    icase = True


def _kind(name, ref_cls, **kw):
    return Kind(name, ref_cls,
                ids=lambda r, b: r.search_any_ids_batch(b, **kw),
                packed=lambda r, b: r.search_any_batch_packed(b, **kw),
                counts=lambda r, b: r.count_any_bytes(b, **kw),
                rows=_listed, want=lambda ref, s: ref.search_any_ids(s), ordered=lambda ref, s: ref.ordered_ids(s),
                want_hits=lambda ref, b: ref.hits(b))


ANY = _kind('any', AnyRef)
ANY_ICASE = _kind('any_icase', AnyIcaseRef, icase=True)
