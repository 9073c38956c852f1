"""pysubstringsearch_amd -- MI355X-native drop-in for ``pysubstringsearch``.

Same classes, method names, argument names and error behaviour as the
reference Python layer (pysubstringsearch/__init__.py:6-73 over
src/lib.rs:42-288); the work is done by hand-written HIP kernels for gfx950
behind the C ABI of ``libpss.so`` (include/pss.h):

* ``Writer`` builds each chunk's 32-bit suffix array on the GPU and writes the
  reference's ``.idx`` chunk records byte for byte.
* ``Reader`` keeps text and suffix arrays resident in HBM;
  ``search_multiple`` is ONE batched device call (one wavefront per query)
  instead of a Python loop.

Extras that do not change the reference signatures: ``device=`` keyword,
``close()`` / context-manager support, ``Reader(..., shard=(i, n))``.
"""
import ctypes
import functools
import os
import typing

from . import _ffi
from ._ffi import lib as _lib

try:   # C loop for result lists (csrc/pyglue.c); plain Python slicing if it was not built
    from . import _pssglue
except ImportError:   # pragma: no cover
    _pssglue = None

__all__ = ['Writer', 'Reader', 'PackedResult', 'IdResult', 'DeviceResult', 'device_count', 'default_devices', 'release_workspace', 'workspace_bytes',
           'glob_parse', 'glob_escape', 'glob_cores', 'icase_variants', 'near_pieces', 'near_seeds', 'any_alternatives',
           'regex_literals', 'regex_info', 'regex_match', 'regex_escape']


def device_count() -> int:
    return _lib.pss_device_count()


def release_workspace() -> None:
    """Free the engine's grow-only HBM workspace (suffix-array build buffers, search
    scratch) on every device; resident Reader chunks stay."""
    _ffi.check(_lib.pss_release_workspace())


def workspace_bytes(device: int = 0) -> int:
    """HBM the engine's grow-only workspaces of ``device`` hold right now (include/pss.h, pss_workspace_bytes): what a
    chunk in flight costs next to a resident Reader; ``release_workspace()`` gives it back."""
    return int(_lib.pss_workspace_bytes(int(device)))


def default_devices() -> typing.List[int]:
    """The devices ``Reader(path)`` / ``Writer(path)`` use when neither ``device`` nor ``devices`` is given
    (include/pss.h, pss_default_devices): ``PSS_DEVICES=all|0,1,...``; else the one a launcher pinned this process to
    (``PSS_DEVICE`` / ``LOCAL_RANK`` / ``SLURM_LOCALID`` / ``OMPI_COMM_WORLD_LOCAL_RANK``); else every visible device -- the reference's ``search`` uses every core of the
    machine without being asked (src/lib.rs:205-207)."""
    arr = (ctypes.c_int32 * 64)()
    k = _lib.pss_default_devices(arr, 64)
    if k < 1:
        raise ValueError(_ffi.last_error() or 'PSS_DEVICES does not name devices')
    return [int(arr[i]) for i in range(k)]


def _default_device() -> int:
    return default_devices()[0]


def _utf8(value, name: str) -> bytes:
    # pyo3 `&str` extraction: only str is accepted (bytes -> TypeError)
    if not isinstance(value, str):
        raise TypeError(f"argument '{name}': '{type(value).__name__}' object cannot be converted to 'PyString'")
    return value.encode('utf-8')


def _path(value, name: str) -> bytes:
    if not isinstance(value, str):
        raise TypeError(f"argument '{name}': '{type(value).__name__}' object cannot be converted to 'PyString'")
    return os.fsencode(value)


def _pack_queries(patterns: typing.Sequence[bytes]):
    """(blob, offsets) of one batch as the C calls take it: the patterns back to back and their nq + 1 offsets (numpy uint64)."""
    import numpy as np
    nq = len(patterns)
    offs = np.zeros(nq + 1, dtype=np.uint64)
    if nq:
        np.cumsum(np.fromiter(map(len, patterns), dtype=np.uint64, count=nq), out=offs[1:])
    return b''.join(patterns), offs


def glob_parse(pattern: bytes, classes: bool = False, *, fold: bool = False):
    """``(segments, anchors)`` of a glob pattern as ``Reader.search_glob_ids_batch`` searches it (include/pss.h,
    pss_reader_search_seq_batch).  ``*`` stands for any run of bytes, also none; ``\\`` takes the next byte literally
    (``\\*``, ``\\\\``); adjacent ``*`` are one.  The anchors follow from the pattern's ends: no unescaped ``*`` in front sets
    ``PSS_ANCHOR_START`` (1), none behind sets ``PSS_ANCHOR_END`` (2).  ``ValueError`` for a lone ``\\`` at the end and for a
    pattern without a literal byte.  Pure Python: no device is touched.

    ``classes=True``: ``?`` is exactly one byte of the entry, ``[set]`` one byte out of ``set`` and ``[!set]`` one byte not in
    it (only ``!`` negates: ``^`` is a member, as in ``fnmatch``); ``a-z`` inside brackets is an inclusive byte range, a ``]``
    right behind ``[`` or ``[!`` and a ``-`` first or last are members, and ``\\`` takes the next byte literally inside
    brackets too.  A segment is then a LIST with one ``bytes`` object per position: the sorted bytes the position accepts --
    one byte for a literal (so ``[*]`` is a literal), the 255 bytes other than newline for ``?``.  ``0x0A`` is taken out of
    every set: an entry holds none.  ``ValueError`` also for an unclosed ``[``, an empty set, a descending range and a
    pattern none of whose segments holds a literal byte (``glob_cores``).  ``fold=True`` (with ``classes``) shows the sets as
    ``icase=True`` searches them: what is written between the brackets is closed under the ASCII fold before ``!`` negates,
    so ``[a-c]`` accepts ``B`` and ``[!a]`` rejects ``A``; literals, a set of one byte among them, stay as written (the
    search folds them), so a pattern has the same cores with and without fold.  ``classes=False`` is the parser as it
    always was."""
    if not isinstance(pattern, (bytes, bytearray)):
        raise TypeError(f'a glob pattern must be bytes, not {type(pattern).__name__}')
    pattern = bytes(pattern)
    if classes:
        return _glob_parse_classes(pattern, bool(fold))
    segments: typing.List[bytes] = []
    cur = bytearray()
    first_star = last_star = False
    i, n = 0, len(pattern)
    while i < n:
        c = pattern[i]
        if c == 0x2A:                               # '*': closes the segment before it
            if cur:
                segments.append(bytes(cur))
                cur = bytearray()
            elif not segments:
                first_star = True
            last_star = True
            i += 1
            continue
        if c == 0x5C:                               # '\\': the next byte as it is
            if i + 1 >= n:
                raise ValueError(f'glob pattern {pattern!r} ends in a lone backslash (write it as two)')
            i += 1
            c = pattern[i]
        cur.append(c)
        last_star = False
        i += 1
    if cur:
        segments.append(bytes(cur))
    if not segments:
        raise ValueError(f"glob pattern {pattern!r} has no literal byte: '*' alone matches every entry (entry_counts counts "
                         "them), the empty pattern the empty entries (search_exact(''))")
    return segments, (0 if first_star else _ffi.ANCHOR_START) | (0 if last_star else _ffi.ANCHOR_END)


def glob_escape(text: bytes, classes: bool = False) -> bytes:
    """``text`` with every ``*`` and ``\\`` escaped: ``glob_parse(glob_escape(x)) == ([x], 3)`` for a non-empty ``x``.
    ``classes=True`` also escapes ``?``, ``[`` and ``]``: ``glob_parse(glob_escape(x, classes=True), classes=True)`` is
    ``([[bytes([b]) for b in x]], 3)``."""
    if not isinstance(text, (bytes, bytearray)):
        raise TypeError(f'glob_escape takes bytes, not {type(text).__name__}')
    out = bytes(text).replace(b'\\', b'\\\\').replace(b'*', b'\\*')
    if classes:
        out = out.replace(b'?', b'\\?').replace(b'[', b'\\[').replace(b']', b'\\]')
    return out


_ANY_BYTE = bytes(b for b in range(256) if b != 0x0A)     # what ``?`` accepts


def _fold_closed(members: typing.Set[int]) -> typing.Set[int]:
    """members and, for every ASCII letter among them, the letter's other case."""
    return members | {b ^ 0x20 for b in members if 0x41 <= (b & 0xDF) <= 0x5A}


def _glob_set(pattern: bytes, i: int, fold: bool) -> typing.Tuple[bytes, int]:
    """(accepted bytes, index behind the closing ``]``) of the bracket expression whose ``[`` stands at pattern[i]."""
    n = len(pattern)
    j = i + 1
    negate = j < n and pattern[j] == 0x21           # '!'
    if negate:
        j += 1
    members: typing.Set[int] = set()
    first = True

    def item(j):                                    # one member byte at j, escaped or not -> (byte, index behind it)
        if j >= n:
            raise ValueError(f'glob pattern {pattern!r}: the [ at byte {i} is not closed')
        if pattern[j] == 0x5C:
            if j + 1 >= n:
                raise ValueError(f'glob pattern {pattern!r} ends in a lone backslash (write it as two)')
            return pattern[j + 1], j + 2
        return pattern[j], j + 1

    while True:
        if j >= n:
            raise ValueError(f'glob pattern {pattern!r}: the [ at byte {i} is not closed')
        if pattern[j] == 0x5D and not first:        # ']' (right behind '[' or '[!' it is a member)
            j += 1
            break
        first = False
        lo, j = item(j)
        if j + 1 < n and pattern[j] == 0x2D and pattern[j + 1] != 0x5D:     # 'lo-hi' (a '-' in front of ']' is a member)
            hi, j = item(j + 1)
            if hi < lo:
                raise ValueError(f'glob pattern {pattern!r}: the range {bytes([lo])!r}-{bytes([hi])!r} descends')
            members.update(range(lo, hi + 1))
        else:
            members.add(lo)
    if fold and (negate or len(members) > 1):       # (one byte is a literal, which folds as every literal does: the cores stay
        members = _fold_closed(members)             # the same with and without fold)
    if negate:
        members = set(range(256)) - members
    members.discard(0x0A)
    if not members:
        raise ValueError(f'glob pattern {pattern!r}: the set at byte {i} is empty (no byte of an entry is in it)')
    return bytes(sorted(members)), j


def _glob_parse_classes(pattern: bytes, fold: bool):
    """``glob_parse(pattern, classes=True)``: segments as lists of byte sets."""
    segments: typing.List[typing.List[bytes]] = []
    cur: typing.List[bytes] = []
    first_star = last_star = False
    i, n = 0, len(pattern)
    while i < n:
        c = pattern[i]
        if c == 0x2A:                               # '*': closes the segment before it
            if cur:
                segments.append(cur)
                cur = []
            elif not segments:
                first_star = True
            last_star = True
            i += 1
            continue
        last_star = False
        if c == 0x5C:                               # '\\': the next byte as it is
            if i + 1 >= n:
                raise ValueError(f'glob pattern {pattern!r} ends in a lone backslash (write it as two)')
            cur.append(pattern[i + 1:i + 2])
            i += 2
        elif c == 0x3F:                             # '?'
            cur.append(_ANY_BYTE)
            i += 1
        elif c == 0x5B:                             # '['
            members, i = _glob_set(pattern, i, fold)
            cur.append(members)
        else:
            cur.append(pattern[i:i + 1])
            i += 1
    if cur:
        segments.append(cur)
    if not any(len(pos) == 1 for seg in segments for pos in seg):
        raise ValueError(f"glob pattern {pattern!r} has no literal byte: nothing in the suffix array can be looked up for it "
                         "('*' alone matches every entry, entry_counts counts them)")
    return segments, (0 if first_star else _ffi.ANCHOR_START) | (0 if last_star else _ffi.ANCHOR_END)


def _segment_core(seg: typing.Sequence[bytes]) -> typing.Optional[typing.Tuple[int, bytes]]:
    """The core of one segment of ``glob_parse(..., classes=True)``: (offset, bytes) of its longest run of literal positions,
    the leftmost on a tie; None for a segment without one."""
    best_off = best_len = 0
    i, n = 0, len(seg)
    while i < n:
        if len(seg[i]) != 1:
            i += 1
            continue
        j = i
        while j < n and len(seg[j]) == 1:
            j += 1
        if j - i > best_len:
            best_off, best_len = i, j - i
        i = j
    return (best_off, b''.join(seg[best_off:best_off + best_len])) if best_len else None


def glob_cores(pattern: bytes) -> typing.List[typing.Optional[typing.Tuple[int, bytes]]]:
    """Per segment of ``glob_parse(pattern, classes=True)`` its CORE as ``(offset, bytes)``: the longest run of literal
    positions, the leftmost on a tie -- what ``Reader.search_glob_ids_batch(..., classes=True)`` looks up in the suffix
    arrays for the segment (include/pss.h, pss_reader_search_seqc_batch).  A segment without a literal position (``??``,
    ``[0-9]``) has no core: ``None``.  The rarest core of every (pattern, chunk) pair drives the search, so ``hits`` and the
    order of the result follow from this rule.  Host only: no device is touched."""
    return [_segment_core(seg) for seg in glob_parse(pattern, classes=True)[0]]


def icase_variants(pattern: bytes, letters: typing.Optional[int] = None) -> typing.Tuple[int, typing.List[bytes]]:
    """``(seed_off, variants)`` of a pattern as ``Reader.search_icase_ids_batch`` searches it (include/pss.h,
    pss_icase_variants): the SEED is the pattern's longest window with at most ``letters`` ASCII letters (1 .. 6; ``None`` =
    the configured ``PSS_ICASE_SEED_LETTERS``, default 5), the leftmost on a tie, ``seed_off`` its offset in the pattern, and
    ``variants`` its ``2**f`` spellings in ascending byte order.  Only the ASCII letters ``A-Z`` / ``a-z`` fold; every other
    byte, ``0x80 .. 0xFF`` included, stands for itself.  ``ValueError`` for an empty pattern and for ``letters`` outside
    1 .. 6.  Host only: no device is touched."""
    if not isinstance(pattern, (bytes, bytearray)):
        raise TypeError(f'a pattern must be bytes, not {type(pattern).__name__}')
    if letters is not None and not 1 <= int(letters) <= 6:
        raise ValueError(f'letters = {letters!r}: 1 .. 6, or None for PSS_ICASE_SEED_LETTERS')
    pattern = bytes(pattern)
    want = 0 if letters is None else int(letters)
    off, ln, cnt = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _ffi.check(_lib.pss_icase_variants(pattern, len(pattern), want, None, 0, ctypes.byref(off), ctypes.byref(ln), ctypes.byref(cnt)))
    buf = ctypes.create_string_buffer(max(1, ln.value * cnt.value))
    _ffi.check(_lib.pss_icase_variants(pattern, len(pattern), want, buf, ln.value * cnt.value, ctypes.byref(off), ctypes.byref(ln),
                                       ctypes.byref(cnt)))
    raw = buf.raw
    return int(off.value), [raw[i * ln.value:(i + 1) * ln.value] for i in range(cnt.value)]


class _Regex:
    """One compiled pattern (``pss_regex_compile``), freed with the object."""

    def __init__(self, pattern, icase) -> None:
        pattern = _regex_bytes(pattern)
        flags = _ffi.REGEX_ICASE if _icase_flag(icase) else 0
        self.handle = ctypes.c_void_p()
        _ffi.check(_lib.pss_regex_compile(pattern, len(pattern), flags, ctypes.byref(self.handle)))

    def __del__(self):
        if getattr(self, 'handle', None):
            _lib.pss_regex_free(self.handle)
            self.handle = None


def _regex_bytes(pattern) -> bytes:
    """A regex pattern as bytes: ``bytes`` as they are, ``str`` UTF-8 encoded."""
    if isinstance(pattern, str):
        return _utf8(pattern, 'pattern')
    if not isinstance(pattern, (bytes, bytearray)):
        raise TypeError(f"argument 'pattern': must be bytes or str, not {type(pattern).__name__}")
    return bytes(pattern)


def regex_literals(pattern, icase: bool = False) -> typing.List[bytes]:
    """The REQUIRED LITERALS of a regex pattern, as ``Reader.search_regex_ids_batch`` looks them up: byte runs every match
    holds, the longest first (the leftmost on a tie), at most 8, folded to lower case under ``icase``.  The rarest of them
    per (pattern, chunk) drives the search.  ``ValueError`` for a pattern the search refuses (include/pss.h,
    pss_regex_compile).  Host only."""
    rx = _Regex(pattern, icase)
    offs = (ctypes.c_uint64 * 9)()
    count = ctypes.c_uint32()
    _ffi.check(_lib.pss_regex_literals(rx.handle, None, 0, offs, ctypes.byref(count)))       # the sizes: a literal may outgrow its pattern
    cap = max(int(offs[count.value]), 1)
    out = ctypes.create_string_buffer(cap)
    _ffi.check(_lib.pss_regex_literals(rx.handle, out, cap, offs, ctypes.byref(count)))
    return [out.raw[offs[i]:offs[i + 1]] for i in range(count.value)]


def regex_info(pattern, icase: bool = False) -> dict:
    """What a regex pattern compiles to: ``states`` and ``classes`` of its DFA, ``table_bytes``, ``anchors`` (1 = ``^``,
    2 = ``$``), the ``start`` state, ``first_accept`` (the accepting states are the ones from it on; 0 is dead) and ``sink``
    (the one absorbing accepting state of a pattern without ``$``; 0: none).  Host only."""
    rx = _Regex(pattern, icase)
    info = _ffi.RegexDfa()
    _ffi.check(_lib.pss_regex_info(rx.handle, ctypes.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in info._fields_}


def regex_match(pattern, data: bytes, icase: bool = False) -> bool:
    """Does ``data``, taken as ONE ENTRY (it holds no newline), match the regex pattern?  The walk the device makes, on
    the host: ``re.search(pattern, data, re.I if icase else 0) is not None`` for every pattern of the subset."""
    rx = _Regex(pattern, icase)
    if not isinstance(data, (bytes, bytearray)):
        raise TypeError(f"argument 'data': must be bytes, not {type(data).__name__}")
    data = bytes(data)
    rc = _lib.pss_regex_match(rx.handle, data, len(data))
    if rc < 0:
        _ffi.check(rc)
    return bool(rc)


_REGEX_SPECIAL = frozenset(b'\\.^$*+?{}[]()|')


def regex_escape(text: bytes) -> bytes:
    """``text`` as a regex pattern that matches exactly these bytes (``str`` is UTF-8 encoded first)."""
    text = _regex_bytes(text)
    return b''.join(b'\\' + bytes([b]) if b in _REGEX_SPECIAL else (b'\\n' if b == 0x0A else bytes([b])) for b in text)


def near_pieces(pattern: bytes, k: int) -> typing.List[typing.Tuple[int, bytes]]:
    """``[(offset, piece), ...]`` of a pattern as ``Reader.search_near_ids_batch`` searches it within ``k`` mismatches
    (include/pss.h, pss_near_pieces): the ``k + 1`` non-empty pieces ``pattern[j * L // (k + 1) : (j + 1) * L // (k + 1)]``,
    left to right.  ``k`` mismatches cannot touch all of them, so every window within budget holds one piece exactly, at
    its offset.  ``ValueError`` for an empty pattern, for ``k`` outside 0 .. 3 and for a pattern of at most ``k`` bytes.
    Host only: no device is touched."""
    if not isinstance(pattern, (bytes, bytearray)):
        raise TypeError(f'a pattern must be bytes, not {type(pattern).__name__}')
    k = _near_budget(k)
    pattern = bytes(pattern)
    off, ln, cnt = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
    _ffi.check(_lib.pss_near_pieces(pattern, len(pattern), k, off, ln, ctypes.byref(cnt)))
    return [(int(off[j]), pattern[off[j]:off[j] + ln[j]]) for j in range(cnt.value)]


def near_seeds(pattern: bytes, k: int, letters: typing.Optional[int] = None) -> typing.List[typing.Tuple[int, int, bytes]]:
    """``[(piece, pos, bytes), ...]``: the seed queries of a pattern as ``Reader.search_near_ids_batch(..., icase=True)``
    searches it within ``k`` mismatches or edits (include/pss.h, pss_near_seeds), in the order of the search.  Every piece
    of ``near_pieces(pattern, k)`` is looked up as a case-insensitive term is: through the spellings, ascending, of its
    SEED -- the piece's longest window with at most ``f`` ASCII letters, the leftmost on a tie.  ``piece`` is the piece's
    index and ``pos`` the seed's position inside the pattern.  ``f`` is ``letters`` (1 .. 6; ``None`` = the configured
    ``PSS_ICASE_SEED_LETTERS``) but at most 6, 5, 4, 4 for ``k`` = 0 .. 3, so that a pattern has at most 64 queries.
    ``ValueError`` as for ``near_pieces``, and for ``letters`` outside 1 .. 6.  Host only: no device is touched."""
    if not isinstance(pattern, (bytes, bytearray)):
        raise TypeError(f'a pattern must be bytes, not {type(pattern).__name__}')
    k = _near_budget(k)
    if letters is not None and not 1 <= int(letters) <= 6:
        raise ValueError(f'letters = {letters!r}: 1 .. 6, or None for PSS_ICASE_SEED_LETTERS')
    pattern = bytes(pattern)
    want = 0 if letters is None else int(letters)
    piece, pos, ln, cnt = (ctypes.c_uint32 * 64)(), (ctypes.c_uint32 * 64)(), (ctypes.c_uint32 * 64)(), ctypes.c_uint32()
    _ffi.check(_lib.pss_near_seeds(pattern, len(pattern), k, want, None, 0, piece, pos, ln, ctypes.byref(cnt)))
    total = sum(ln[v] for v in range(cnt.value))
    buf = ctypes.create_string_buffer(max(1, total))
    _ffi.check(_lib.pss_near_seeds(pattern, len(pattern), k, want, buf, total, piece, pos, ln, ctypes.byref(cnt)))
    raw, out, at = buf.raw, [], 0
    for v in range(cnt.value):
        out.append((int(piece[v]), int(pos[v]), raw[at:at + ln[v]]))
        at += ln[v]
    return out


def _any_set(alts, where: str) -> typing.List[bytes]:
    """One any-of set as a list of ``bytes``: ``TypeError`` for a bare ``bytes`` / ``str`` in the sequence's place (it would
    be read as its characters) and for a member that is not ``bytes``, ``ValueError`` for an empty set or alternative."""
    if isinstance(alts, (bytes, bytearray, str)):
        raise TypeError(f"{where}: '{type(alts).__name__}' object cannot be converted to a sequence of alternatives")
    alts = list(alts)
    for a in alts:
        if not isinstance(a, (bytes, bytearray)):
            raise TypeError(f'{where}: an alternative must be bytes, not {type(a).__name__}')
        if len(a) == 0:
            raise ValueError(f'{where}: an empty alternative (every entry contains it)')
    if not alts:
        raise ValueError(f'{where}: no alternative (a set without one matches nothing: leave it out)')
    return [bytes(a) for a in alts]


def any_alternatives(terms: typing.Sequence[bytes], icase: bool = False,
                     letters: typing.Optional[int] = None) -> typing.List[typing.Tuple[bytes, int, bytes]]:
    """``[(alternative, seed_position, seed_bytes), ...]``: one any-of set as ``Reader.search_any_ids_batch`` asks the
    device for it (include/pss.h, pss_any_alternatives).  The set is NORMALISED: under ``icase`` folded to lower case
    (``A-Z`` alone), duplicates dropped, every alternative with a newline dropped (it occurs in no entry; it voids itself,
    not its set), every alternative that holds another one as a substring dropped, the rest ascending bytewise -- what is
    left is prefix-free.  Exact: every alternative is one query, ``seed_position`` 0 and ``seed_bytes`` the alternative.
    Under ``icase`` an alternative is looked up through the spellings (``icase_variants``) of its SEED ``seed_bytes`` at
    ``seed_position`` inside it: the longest window with at most ``F`` ASCII letters, the leftmost on a tie, ``F`` =
    ``letters`` (1 .. 6; ``None`` = the configured ``PSS_ICASE_SEED_LETTERS``) but at most ``floor(log2(64 / len(result)))``,
    so that a set has at most 64 queries.  ``ValueError`` for an empty set, an empty alternative, more than 64 alternatives
    after normalisation (32 under ``icase``) and ``letters`` outside 1 .. 6; ``TypeError`` for a member that is not
    ``bytes`` and an ``icase`` that is not a bool.  Host only: no device is touched."""
    import numpy as np
    flags = _ffi.ANY_ICASE if _icase_flag(icase) else 0
    alts = _any_set(terms, 'any_alternatives')
    if letters is not None and not 1 <= int(letters) <= 6:
        raise ValueError(f'letters = {letters!r}: 1 .. 6, or None for PSS_ICASE_SEED_LETTERS')
    blob, offs = _pack_queries(alts)
    n = len(alts)
    out = ctypes.create_string_buffer(max(1, len(blob)))
    ooff, pos, ln = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    cnt = ctypes.c_uint32()
    _ffi.check(_lib.pss_any_alternatives(blob, offs.ctypes.data, n, flags, 0 if letters is None else int(letters), out, len(blob),
                                         ooff.ctypes.data, pos.ctypes.data, ln.ctypes.data, ctypes.byref(cnt)))
    raw, res = out.raw, []
    for j in range(cnt.value):
        alt = raw[int(ooff[j]):int(ooff[j + 1])]
        res.append((alt, int(pos[j]), alt[int(pos[j]):int(pos[j]) + int(ln[j])]))
    return res


def _near_budget(k) -> int:
    """One mismatch budget: an int in 0 .. 3 (a bool, a float or a pattern in its place is a ``TypeError``)."""
    if isinstance(k, bool) or not hasattr(k, '__index__'):
        raise TypeError(f'a mismatch budget k must be an int, not {type(k).__name__}')
    k = k.__index__()
    if not 0 <= k <= 3:
        raise ValueError(f'k = {k}: a mismatch budget is 0 .. 3')
    return int(k)


class Writer:
    """Reference: pysubstringsearch/__init__.py:6-41, src/lib.rs:42-144."""

    def __init__(
        self,
        index_file_path: str,
        max_chunk_len: typing.Optional[int] = None,
        *,
        device: typing.Optional[int] = None,
        devices: typing.Optional[typing.Sequence[int]] = None,
        format_version: int = 1,
        striped: bool = False,
    ) -> None:
        """``format_version=2`` (extension, opt-in) writes the container with 64-bit lengths: chunks of
        up to 2^31 - 1 bytes instead of the reference format's < 1 GiB.  Reader opens either.
        ``striped=True`` (with ``format_version=2``) keeps the suffix arrays out of the index file, in eight files
        ``<path>.sa0 .. .sa7`` written and read by a thread each (include/pss.h, PSS_FORMAT_STRIPED): one file in the
        page cache takes 11 - 14 GB/s on the test box however many threads write it, a file per writer four times that.
        ``devices=[0, 1, ...]`` (extension) builds chunk k of the file on ``devices[k % len(devices)]``,
        several chunks at once; the records are still written in chunk order, so the file is
        byte-identical to the single-device one."""
        if format_version not in (1, 2):
            raise ValueError('format_version must be 1 (the reference container) or 2')
        if striped and format_version != 2:
            raise ValueError('striped=True needs format_version=2 (the reference container has no place for the flag)')
        if max_chunk_len is not None:
            if not isinstance(max_chunk_len, int) or isinstance(max_chunk_len, bool):
                raise TypeError("argument 'max_chunk_len': must be an int or None")
            if max_chunk_len < 0:
                raise OverflowError("can't convert negative int to unsigned")   # Option<usize>
        self._h = ctypes.c_void_p()
        path = _path(index_file_path, 'index_file_path')
        if devices is not None:
            if device is not None:
                raise ValueError('pass either device or devices')
            devs = [int(d) for d in devices]
            if not devs:
                raise ValueError('devices must not be empty')
        else:
            devs = default_devices() if device is None else [device]      # no argument: every device the process may use
        self.devices = list(devs)
        arr = (ctypes.c_int32 * len(devs))(*devs)
        rc = _lib.pss_writer_open_multi(
            path, -1 if max_chunk_len is None else max_chunk_len, arr, len(devs), format_version | (0x100 if striped else 0),
            ctypes.byref(self._h))
        _ffi.check(rc, index_file_path)

    @property
    def writer(self) -> 'Writer':
        """The reference wrapper exposes `.writer` (the native object, __init__.py:12).  A property, not an attribute
        holding `self`: that would make every handle a reference cycle, and `del w` would flush the last chunk only
        when the cyclic collector gets round to it -- the reference's Drop flushes at once (src/lib.rs:138-144)."""
        return self

    def _handle(self):
        if not self._h:
            raise ValueError('I/O operation on closed Writer')
        return self._h

    @property
    def io_stats(self) -> dict:
        """Extension (diagnostics): records written through a shared mapping / pwritten, file-ingest bytes read straight
        into the chunk / through a block buffer (include/pss.h, pss_writer_io_stats)."""
        st = _ffi.WriterIo()
        _ffi.check(_lib.pss_writer_io_stats(self._handle(), ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def add_entries_from_file_lines(self, input_file_path: str) -> None:
        _ffi.check(_lib.pss_writer_add_file_lines(self._handle(), _path(input_file_path, 'input_file_path')),
                   input_file_path)

    def add_entry(self, text: str) -> None:
        b = _utf8(text, 'text')
        _ffi.check(_lib.pss_writer_add_entry(self._handle(), b, len(b)))

    def dump_data(self) -> None:
        _ffi.check(_lib.pss_writer_dump(self._handle()))

    def finalize(self) -> None:
        _ffi.check(_lib.pss_writer_finalize(self._handle()))

    def close(self) -> None:
        """Finalize and release the file (the reference does this on drop, src/lib.rs:138-144)."""
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            _ffi.check(_lib.pss_writer_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ResultOwner:
    """Keeps a pss_result alive for the numpy views handed out by search_batch_packed."""

    def __init__(self, handle) -> None:
        self._h = handle

    def view(self, ptr, count: int, dtype):
        import numpy as np
        if not count or not ptr:
            return np.zeros(0, dtype=dtype)
        nbytes = int(count) * np.dtype(dtype).itemsize
        buf = (ctypes.c_uint8 * nbytes).from_address(ctypes.addressof(ptr.contents))
        buf._owner = self               # numpy keeps `buf` as the array's base, `buf` keeps the result
        a = np.frombuffer(buf, dtype=dtype, count=int(count))
        a.flags.writeable = False
        return a

    def __del__(self):
        h, self._h = self._h, None
        if h:
            _lib.pss_result_free(h)


class PackedResult(typing.NamedTuple):
    data: typing.Any      # numpy uint8: all entries back to back
    offsets: typing.Any   # numpy uint64 [num_entries + 1]
    counts: typing.Any    # numpy uint64 [num_queries]


class IdResult(typing.NamedTuple):
    """Entry ids of one batch (``Reader.search_ids_batch``): ``(chunk index in the file << 32) | line``."""
    ids: typing.Any       # numpy uint64 [num_entries], read-only view of the result, query-major
    counts: typing.Any    # numpy uint64 [num_queries]


class _DevicePtr:
    """A raw HBM range as an object torch.as_tensor understands (CUDA array interface)."""

    def __init__(self, ptr: int, nbytes: int) -> None:
        self.__cuda_array_interface__ = {'shape': (nbytes,), 'typestr': '|u1', 'data': (ptr, False), 'version': 2}


class DeviceResult(typing.NamedTuple):
    """Packed result of one batch left in HBM (torch tensors owned by the caller)."""
    data: typing.Any      # torch uint8 [num_bytes]
    starts: typing.Any    # torch int64 [num_entries]: start of every entry in data
    counts: typing.Any    # torch int64 [num_queries]
    num_bytes: int


def _icase_flag(icase) -> bool:
    """The ``icase`` keyword of the all-terms and the glob calls: a bool and nothing else (a pattern slipped into its place
    is a mistake worth a ``TypeError``)."""
    if not isinstance(icase, bool):
        raise TypeError(f"argument 'icase': must be bool, not {type(icase).__name__}")
    return icase


def _classes_flag(classes) -> bool:
    """The ``classes`` keyword of the glob calls: a bool and nothing else, as ``icase``."""
    if not isinstance(classes, bool):
        raise TypeError(f"argument 'classes': must be bool, not {type(classes).__name__}")
    return classes


def _with_icase(folded, note: str, classed=None):
    """Decorator of the ten all-terms and glob methods of ``Reader``: adds the keyword-only ``icase: bool = False``.
    ``icase=False`` calls the decorated exact-byte method as it stands -- not one line of its path changes; ``icase=True``
    calls ``folded`` with the same arguments.  ``functools.wraps`` keeps the method's name and appends ``note`` to its
    docstring; like every wrapped function it also keeps the exact-byte method's ``inspect.signature`` (``__wrapped__``) --
    the keyword itself is declared in ``__init__.pyi`` and shown by ``inspect.signature(m, follow_wrapped=False)``.
    ``classed`` (the five glob methods): the wrapper also takes the keyword-only ``classes: bool = False``;
    ``classes=True`` calls ``classed(self, *args, icase=...)`` -- the pattern language with ``?`` and ``[...]`` -- and
    ``classes=False`` the two bodies above, exactly as without the keyword."""
    def decorate(exact):
        if classed is None:
            @functools.wraps(exact)
            def method(self, *args, icase: bool = False, **kwargs):
                return (folded if _icase_flag(icase) else exact)(self, *args, **kwargs)
        else:
            @functools.wraps(exact)
            def method(self, *args, icase: bool = False, classes: bool = False, **kwargs):
                if _classes_flag(classes):
                    return classed(self, *args, icase=_icase_flag(icase), **kwargs)
                return (folded if _icase_flag(icase) else exact)(self, *args, **kwargs)
        method.__doc__ = (exact.__doc__ or '') + note
        return method
    return decorate


def _folded_batch(kind: str, form: str):
    """The ``icase=True`` body of one batched method: ``kind`` 'terms' (all-terms groups) or 'seq' (glob patterns), ``form``
    'packed', 'ids' or 'counts'.  The batch is packed exactly as for the exact-byte call (``Reader._terms_args`` /
    ``Reader._glob_args``: the same ``ValueError`` / ``TypeError``) and handed to the ``_icase`` namesake of its C entry point."""
    pack = {'terms': '_terms_args', 'seq': '_glob_args'}[kind]
    name = {'packed': f'pss_reader_search_{kind}_icase_batch', 'ids': f'pss_reader_search_{kind}_icase_ids_batch',
            'counts': f'pss_reader_count_{kind}_icase_batch'}[form]

    def run(self, batch):
        return self._group_batch(name, getattr(self, pack)(batch), form)
    return run


def _packed_strs(p: 'PackedResult') -> typing.List[str]:
    data = p.data.tobytes()
    o = p.offsets.tolist()
    return [data[o[i]:o[i + 1]].decode('utf-8') for i in range(len(o) - 1)]


def _folded_search_all(self, terms, exclude=()):
    return _packed_strs(_folded_batch('terms', 'packed')(self, self._str_terms(terms, exclude)))


def _folded_count_all(self, terms, exclude=()):
    return _folded_batch('terms', 'counts')(self, self._str_terms(terms, exclude))[0]


def _folded_search_glob(self, s):
    return _packed_strs(_folded_batch('seq', 'packed')(self, [_utf8(s, 'pattern')]))


def _folded_count_glob(self, s):
    return _folded_batch('seq', 'counts')(self, [_utf8(s, 'pattern')])[0]


SEQ_MAX_SETS = 255      # distinct byte sets one batch of class globs carries (include/pss.h, pss_reader_search_seqc_batch)


def _glob_class_args(patterns, fold: bool):
    """The arguments of one ``pss_reader_search_seqc_*`` call between the reader and the output: the segments of every
    pattern (``glob_parse(p, classes=True, fold=fold)``) as literal bytes and class plane, the batch's distinct sets as
    256-bit memberships, the group offsets, the anchors and the flags word.  Returns ``(args, keep)``; ``keep`` holds the
    arrays the pointers in ``args`` point into."""
    import numpy as np
    if isinstance(patterns, (bytes, bytearray, str)):
        raise TypeError(f"argument 'patterns': '{type(patterns).__name__}' object cannot be converted to a sequence of glob patterns")
    lit = bytearray()
    plane = bytearray()
    soff, goff = [0], [0]
    anch: typing.List[int] = []
    index: typing.Dict[bytes, int] = {}
    for g, pat in enumerate(patterns):
        if not isinstance(pat, (bytes, bytearray)):
            raise TypeError(f'pattern {g}: a glob pattern must be bytes, not {type(pat).__name__}')
        segs, a = glob_parse(pat, classes=True, fold=fold)
        for seg in segs:
            for pos in seg:
                if len(pos) == 1:
                    lit.append(pos[0])
                    plane.append(0)
                    continue
                k = index.get(pos)
                if k is None:
                    if len(index) == SEQ_MAX_SETS:
                        raise ValueError(f'pattern {g}: the batch holds more than {SEQ_MAX_SETS} distinct byte sets (the class plane '
                                         f'names a set in one byte): split the batch')
                    k = index[pos] = len(index) + 1
                lit.append(0)
                plane.append(k)
            soff.append(len(lit))
        goff.append(len(soff) - 1)
        anch.append(a)
    sets = np.zeros((max(len(index), 1), 32), dtype=np.uint8)
    for members, k in index.items():
        m = np.frombuffer(members, dtype=np.uint8)
        np.bitwise_or.at(sets[k - 1], m >> 3, np.uint8(1) << (m & 7))
    soffs, goffs = np.array(soff, dtype=np.uint64), np.array(goff, dtype=np.uint64)
    anchors = np.array(anch if anch else [0], dtype=np.uint8)
    keep = (bytes(lit), bytes(plane), soffs, sets, goffs, anchors)
    args = (keep[0], keep[1], soffs.ctypes.data, len(soff) - 1, sets.ctypes.data, len(index), goffs.ctypes.data, len(goff) - 1,
            anchors.ctypes.data, _ffi.SEQ_FOLD if fold else 0)
    return args, keep


def _classed_batch(form: str):
    """The ``classes=True`` body of one batched glob method (``form`` 'packed', 'ids' or 'counts'), exact bytes or under fold."""
    name = {'packed': 'pss_reader_search_seqc_batch', 'ids': 'pss_reader_search_seqc_ids_batch', 'counts': 'pss_reader_count_seqc_batch'}[form]

    def run(self, batch, icase=False):
        args, keep = _glob_class_args(batch, icase)
        return self._batch(getattr(_lib, name), args, args[7], form)
    return run


def _classed_search_glob(self, s, icase=False):
    return _packed_strs(_classed_batch('packed')(self, [_utf8(s, 'pattern')], icase))


def _classed_count_glob(self, s, icase=False):
    return _classed_batch('counts')(self, [_utf8(s, 'pattern')], icase)[0]


_ICASE_ALL = """

        ``icase=True`` (keyword only): every term is compared under ASCII case folding (``A-Z`` = ``a-z``, every other byte
        equals only itself), as ``search_icase_batch_packed`` compares a pattern; the driver of a (group, chunk) pair is then
        the include term whose SEED (``icase_variants``) has the fewest hits, and the entries of a pair come in the
        suffix-array order of that seed's occurrence inside each entry's leftmost folded match of the driver term
        (include/pss.h, pss_reader_search_terms_icase_batch).  ``icase=False`` is the call as it always was."""
_ICASE_GLOB = """

        ``icase=True`` (keyword only): every byte is compared under ASCII case folding (``A-Z`` = ``a-z``, every other byte
        equals only itself): ``grep -i`` for globs.  ``glob_escape(p) + b'*'``, ``b'*' + glob_escape(p)`` and
        ``glob_escape(p)`` are then the case-insensitive "starts with", "ends with" and "equals" (include/pss.h,
        pss_reader_search_seq_icase_batch).  ``icase=False`` is the call as it always was.

        ``classes=True`` (keyword only): ``?`` stands for exactly one byte of the entry and ``[set]`` / ``[!set]`` for one
        byte in / not in a set of bytes (``glob_parse(p, classes=True)`` shows what a pattern stands for, ``glob_escape(x,
        classes=True)`` writes a literal).  A class is one BYTE: ``?`` over UTF-8 text counts bytes.  Every piece between two
        ``*`` is looked up by its CORE, its longest run of literal bytes (``glob_cores``); the rarest core of every (pattern,
        chunk) pair drives and every candidate entry is walked once, left to right (include/pss.h,
        pss_reader_search_seqc_batch).  A pattern needs one literal byte; a batch holds at most 255 distinct sets.  Combines
        with ``icase=True``: a set then accepts both cases of the letters written in it, ``[!a]`` rejects ``A``.
        ``classes=False``, the default, leaves ``?``, ``[`` and ``]`` the literal bytes they always were."""


class Reader:
    """Reference: pysubstringsearch/__init__.py:44-73, src/lib.rs:146-288."""

    def __init__(
        self,
        index_file_path: str,
        *,
        device: typing.Optional[int] = None,
        devices: typing.Optional[typing.Sequence[int]] = None,
        shard: typing.Tuple[int, int] = (0, 1),
        order: typing.Optional[str] = None,
    ) -> None:
        """``order='sa'`` (extension): the entries a chunk contributes to a query come in the reference's order --
        suffix-array order of their first hit, src/lib.rs:262-276 -- so that ``search(s)`` of a one-chunk index equals the
        reference's list element by element (default ``'text'``: the same multiset, see ``set_result_order``).
        ``devices=[0, 1, ...]`` (extension) makes chunk c of the file resident on ``devices[c % len(devices)]`` and
        answers every search on all of them at once, inside this process -- no launcher, no ``torch.distributed``: one
        host thread per device, results merged on the host (the reference fans a search over its chunks with rayon,
        src/lib.rs:207).  ``shard=(i, n)`` is the one-process-per-GPU form of the same split (``dist.ShardedReader``)."""
        self._h = ctypes.c_void_p()
        path = _path(index_file_path, 'index_file_path')
        if devices is not None:
            if device is not None or tuple(shard) != (0, 1):
                raise ValueError('pass devices, or device / shard')
            devs = [int(d) for d in devices]
            if not devs:
                raise ValueError('devices must not be empty')
        elif device is None and tuple(shard) == (0, 1):
            devs = default_devices()        # no argument: every device the process may use (one under a launcher)
        else:
            devs = [_default_device() if device is None else int(device)]
        self.devices = list(devs)
        if len(devs) > 1:
            arr = (ctypes.c_int32 * len(devs))(*devs)
            rc = _lib.pss_reader_open_multi(path, arr, len(devs), ctypes.byref(self._h))
        else:
            rc = _lib.pss_reader_open(path, devs[0], shard[0], shard[1], ctypes.byref(self._h))
        _ffi.check(rc, index_file_path)
        if order is not None:
            self.set_result_order(order)

    @property
    def reader(self) -> 'Reader':
        """The reference wrapper exposes `.reader` (__init__.py:49); a property for the reason given at Writer.writer
        (a dropped Reader gives its HBM back at once)."""
        return self

    @classmethod
    def _from_handle(cls, handle) -> 'Reader':
        r = cls.__new__(cls)
        r._h = handle
        r.devices = []
        return r

    def _handle(self):
        if not self._h:
            raise ValueError('I/O operation on closed Reader')
        return self._h

    @property
    def num_chunks(self) -> int:
        return _lib.pss_reader_num_chunks(self._handle())

    @property
    def chunks_per_device(self) -> typing.List[int]:
        """Extension: how many chunks every part of the reader holds -- chunk c of the file lives on ``devices[c % G]``
        (SURVEY 8(e)), so 15 chunks over 8 devices read ``[2, 2, 2, 2, 2, 2, 2, 1]``; one number for a single-device reader."""
        g = int(_lib.pss_reader_part_chunks(self._handle(), None, 0))
        buf = (ctypes.c_uint64 * max(g, 1))()
        _lib.pss_reader_part_chunks(self._handle(), buf, g)
        return [int(buf[i]) for i in range(g)]

    @property
    def residency(self) -> dict:
        """Extension: where the resident index lives -- bytes in HBM, bytes of suffix arrays kept in
        pinned host memory (chunks beyond the HBM budget) and how many chunks that concerns."""
        hbm, host, nhost = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _ffi.check(_lib.pss_reader_residency(self._handle(), ctypes.byref(hbm), ctypes.byref(host), ctypes.byref(nhost)))
        return {'hbm_bytes': hbm.value, 'host_bytes': host.value, 'host_chunks': nhost.value}

    @property
    def chunk_tiers(self) -> typing.List[str]:
        """Extension: where the suffix array of every chunk lives right now -- 'hbm' or 'host' (pinned memory)."""
        n = self.num_chunks
        buf = (ctypes.c_uint8 * max(n, 1))()
        _ffi.check(_lib.pss_reader_chunk_tiers(self._handle(), buf, n, None))
        return ['host' if buf[i] else 'hbm' for i in range(n)]

    @property
    def residency_moves(self) -> int:
        """Extension: exchanges / promotions the residency manager has made on its own (pss_reader_set_auto_residency)."""
        moves = ctypes.c_uint64()
        _ffi.check(_lib.pss_reader_chunk_tiers(self._handle(), None, 0, ctypes.byref(moves)))
        return moves.value

    def set_auto_residency(self, on: bool = True) -> None:
        """Extension: between batches the hottest suffix array of the host tier changes places with
        the coldest one in HBM (include/pss.h).  On by default; ``evict`` / ``promote`` override by hand."""
        _ffi.check(_lib.pss_reader_set_auto_residency(self._handle(), 1 if on else 0))

    def evict(self, chunk: int) -> None:
        """Extension: move the suffix array of resident chunk ``chunk`` out of HBM into pinned host
        memory (searches keep working, the kernels read it over PCIe); ``promote`` brings it back."""
        _ffi.check(_lib.pss_reader_evict_chunk(self._handle(), int(chunk)))

    def promote(self, chunk: int) -> None:
        _ffi.check(_lib.pss_reader_promote_chunk(self._handle(), int(chunk)))

    def set_result_order(self, order: str) -> None:
        """Extension: ``'sa'`` -- the reference's order inside a chunk (suffix-array order of every entry's first hit,
        src/lib.rs:262-276); ``'text'`` (default) -- suffix-array order of every entry's leftmost match.  The multiset is
        the same; they differ when an entry holds the pattern more than once.  ``PSS_RESULT_ORDER=sa`` sets the default."""
        if order not in ('sa', 'text'):
            raise ValueError("order must be 'sa' or 'text'")
        _ffi.check(_lib.pss_reader_set_result_order(self._handle(), 1 if order == 'sa' else 0))

    @property
    def result_order(self) -> str:
        return 'sa' if _lib.pss_reader_result_order(self._handle()) == 1 else 'text'

    def set_low_latency(self, on: bool = True) -> None:
        """Extension: single queries (``search``) through a resident search kernel that waits for them in a pinned
        mailbox -- no kernel launch, no stream synchronisation per query; same results.  The kernel leaves by itself
        1 ms after the last query (include/pss.h, pss_reader_set_low_latency).  Off by default."""
        _ffi.check(_lib.pss_reader_set_low_latency(self._handle(), 1 if on else 0))

    def low_latency_stats(self) -> dict:
        launches, served = ctypes.c_uint64(), ctypes.c_uint64()
        _ffi.check(_lib.pss_reader_low_latency_stats(self._handle(), ctypes.byref(launches), ctypes.byref(served)))
        return {'kernels_started': launches.value, 'queries_served': served.value}

    def _batch(self, call, args, nrows: int, form: str):
        """One batched C call ``call(handle, *args, out)`` and its result of ``nrows`` rows (queries, groups or ids) in the
        given ``form``: 'packed' -> ``PackedResult``, 'ids' -> ``IdResult``, 'counts' -> a list of int."""
        import numpy as np
        if form == 'counts':
            counts = np.zeros(max(nrows, 1), dtype=np.uint64)
            _ffi.check(call(self._handle(), *args, counts.ctypes.data))
            return [int(c) for c in counts[:nrows]]
        res = ctypes.c_void_p()
        _ffi.check(call(self._handle(), *args, ctypes.byref(res)))
        owner = _ResultOwner(res)      # the arrays below are views of the C result; it lives as long as they do
        n = _lib.pss_result_num_entries(res)
        counts = owner.view(_lib.pss_result_query_counts(res), nrows, np.uint64)
        if form == 'ids':
            ids = owner.view(_lib.pss_result_bytes(res), 8 * n, np.uint8).view(np.uint64)
            ids.flags.writeable = False     # (also the empty array of a batch without entries, which views nothing)
            return IdResult(ids, counts)
        offsets = owner.view(_lib.pss_result_offsets(res), n + 1, np.uint64)
        data = owner.view(_lib.pss_result_bytes(res), int(offsets[n]), np.uint8)
        return PackedResult(data, offsets, counts)

    def _query_batch(self, name: str, packed, form: str, *extra):
        """``_batch`` of the C call ``name`` over ``packed`` = (blob, offsets) of nq patterns, ``extra`` arrays behind them."""
        blob, offs = packed
        nq = len(offs) - 1
        return self._batch(getattr(_lib, name), (blob, offs.ctypes.data, nq) + tuple(a.ctypes.data for a in extra), nq, form)

    def _group_batch(self, name: str, packed, form: str):
        """``_batch`` of the C call ``name`` over ``packed`` = (blob, offsets, group offsets, flags per term or group)."""
        blob, offs, goff, extra = packed
        ng = len(goff) - 1
        return self._batch(getattr(_lib, name), (blob, offs.ctypes.data, len(offs) - 1, goff.ctypes.data, ng, extra.ctypes.data), ng, form)

    def _search_batch(self, patterns: typing.Sequence[bytes], as_str: bool):
        nq = len(patterns)
        if _pssglue is not None:
            blob, offs = _pssglue.pack_queries(patterns)      # one C loop: blob + u64 offsets
        else:
            blob = b''.join(patterns)
            arr = (ctypes.c_uint64 * (nq + 1))()
            pos = 0
            for i, p in enumerate(patterns):
                arr[i] = pos
                pos += len(p)
            arr[nq] = pos
            offs = bytes(arr)
        res = ctypes.c_void_p()
        rc = _lib.pss_reader_search_batch(self._handle(), blob, offs, nq, ctypes.byref(res))
        _ffi.check(rc)
        try:
            n = _lib.pss_result_num_entries(res)
            if not nq:
                counts = []
            elif _pssglue is not None:
                counts = _pssglue.u64_list(ctypes.cast(_lib.pss_result_query_counts(res), ctypes.c_void_p).value, nq)
            else:
                counts = list(_lib.pss_result_query_counts(res)[:nq])
            entries = []
            if n:
                off = _lib.pss_result_offsets(res)
                base = _lib.pss_result_bytes(res)
                if _pssglue is not None:
                    entries = _pssglue.entries_to_list(ctypes.cast(base, ctypes.c_void_p).value,
                                                       ctypes.cast(off, ctypes.c_void_p).value, n, as_str)
                else:
                    # not ctypes.string_at: its size argument is a C int (results beyond 2 GiB)
                    addr = ctypes.cast(base, ctypes.c_void_p).value
                    data = bytes((ctypes.c_char * off[n]).from_address(addr)) if off[n] else b''
                    o = off[:n + 1]
                    entries = [data[o[i]:o[i + 1]] for i in range(n)]
                    if as_str:
                        entries = [e.decode('utf-8') for e in entries]
            return entries, counts
        finally:
            _lib.pss_result_free(res)

    def count_multiple(self, substrings: typing.List[str]) -> typing.List[int]:
        """Extension (not in the reference API): ``len(search(s))`` for every s, in one batched
        device call that materialises no entry -- only the counters come back."""
        import numpy as np
        return self.count_multiple_bytes([_utf8(s, 'substring') for s in substrings])

    def count(self, substring: str) -> int:
        """Extension: ``len(search(substring))`` without building the entries."""
        return self.count_multiple([substring])[0]

    def search_batch_packed(self, patterns: typing.Sequence[bytes]) -> 'PackedResult':
        """One batched device call, zero per-entry Python objects: read-only numpy
        views of the packed result, which lives as long as they do (entry i of the
        batch = data[offsets[i]:offsets[i+1]], entries are query-major, counts[q] of
        them belong to query q).  For
        hit-heavy batches the Python list of ``search_multiple`` costs more than
        the search itself (~50 ns per entry); this is the bulk alternative."""
        return self._query_batch('pss_reader_search_batch', _pack_queries(patterns), 'packed')

    def search_ids_batch(self, patterns: typing.Sequence[bytes]) -> 'IdResult':
        """Extension: WHICH entries match instead of their text -- one ``uint64`` id per entry
        ``search_batch_packed(patterns)`` would return, in the same order (query-major; ``counts[q]`` of them belong to
        query q; each id once per query).  An id is ``(chunk index in the index file << 32) | line``, ``line`` = the
        entry's number inside its chunk; a shard and a multi-device reader hand out the same ids as a whole-file
        reader.  8 bytes per entry come down whatever the entries' length; ``entries_by_id`` fetches the text of the
        ones that are wanted, ``entry_ordinals`` turns ids into positions in the order the entries were added (line
        numbers of the file given to ``add_entries_from_file_lines``)."""
        return self._query_batch('pss_reader_search_ids_batch', _pack_queries(patterns), 'ids')

    def search_ids(self, substring: str):
        """Extension: the ids of the entries ``search(substring)`` returns, in its order (numpy uint64)."""
        return self.search_ids_batch([_utf8(substring, 'substring')]).ids

    def entries_by_id_packed(self, ids) -> 'PackedResult':
        """Extension: the text of the entries ``ids`` (any integer sequence or array; an id may repeat) as a packed
        result -- entry i = ``data[offsets[i]:offsets[i+1]]``, in the order asked, ``counts`` all one.  ``ValueError``
        when an id names a chunk this reader does not hold or a line its chunk does not have."""
        import numpy as np
        arr = np.ascontiguousarray(np.asarray(ids).reshape(-1) if len(ids) else np.zeros(0, dtype=np.uint64))
        if arr.dtype != np.uint64:
            if arr.dtype.kind not in 'iu':
                raise TypeError('entry ids must be integers')
            if arr.dtype.kind == 'i' and arr.size and int(arr.min()) < 0:
                raise ValueError('entry ids are not negative')
            arr = arr.astype(np.uint64)
        n = int(arr.size)
        return self._batch(_lib.pss_reader_entries_by_id, (arr.ctypes.data, n), n, 'packed')

    def entries_by_id(self, ids) -> typing.List[bytes]:
        """Extension: ``entries_by_id_packed`` as a list of byte strings."""
        p = self.entries_by_id_packed(ids)
        data = p.data.tobytes()
        o = p.offsets.tolist()
        return [data[o[i]:o[i + 1]] for i in range(len(o) - 1)]

    @staticmethod
    def _anchored_args(patterns: typing.Sequence[bytes], anchors):
        """(blob, offsets, anchor bytes) of one anchored batch; ``ValueError`` for an anchor that is none of
        ``'start' | 'end' | 'entry'`` or a sequence of another length than ``patterns``."""
        import numpy as np
        nq = len(patterns)
        if isinstance(anchors, str):
            kinds = [anchors] * nq
            if anchors not in _ffi.ANCHORS:
                raise ValueError(f"anchors must be 'start', 'end' or 'entry' (or one of them per pattern), not {anchors!r}")
        else:
            try:
                kinds = list(anchors)
            except TypeError:
                raise ValueError(f"anchors must be 'start', 'end' or 'entry' (or one of them per pattern), not {anchors!r}") from None
        if len(kinds) != nq:
            raise ValueError(f'{len(kinds)} anchors for {nq} patterns')
        for k in kinds:
            if not isinstance(k, str) or k not in _ffi.ANCHORS:
                raise ValueError(f"an anchor is 'start', 'end' or 'entry', not {k!r}")
        blob, offs = _pack_queries(patterns)
        return blob, offs, np.array([_ffi.ANCHORS[k] for k in kinds], dtype=np.uint8)

    def search_anchored_batch_packed(self, patterns: typing.Sequence[bytes], anchors) -> 'PackedResult':
        """Extension: the entries that START WITH (``'start'``), END WITH (``'end'``) or EQUAL (``'entry'``) each
        pattern, as a packed result like ``search_batch_packed``'s.  ``anchors`` is one of the three words for the whole
        batch or a sequence of them, one per pattern.  Exact bytes; every entry at most once per query; the empty
        pattern matches every entry under 'start' and 'end' and the empty entries under 'entry'; a pattern holding a
        newline matches nothing.  The suffix array holds the answer as one interval -- of ``"\\n" + pattern`` and the
        like -- so the work follows the number of matching entries, not of occurrences (include/pss.h)."""
        blob, offs, anc = self._anchored_args(patterns, anchors)
        return self._query_batch('pss_reader_search_anchored_batch', (blob, offs), 'packed', anc)

    def search_anchored_ids_batch(self, patterns: typing.Sequence[bytes], anchors) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_anchored_batch_packed`` returns, in the
        same order."""
        blob, offs, anc = self._anchored_args(patterns, anchors)
        return self._query_batch('pss_reader_search_anchored_ids_batch', (blob, offs), 'ids', anc)

    def count_anchored_bytes(self, patterns: typing.Sequence[bytes], anchors) -> typing.List[int]:
        """Extension: how many entries each pattern matches under its anchor; only the counters come back."""
        blob, offs, anc = self._anchored_args(patterns, anchors)
        return self._query_batch('pss_reader_count_anchored_batch', (blob, offs), 'counts', anc)

    def _search_anchored_str(self, s: str, anchor: str) -> typing.List[str]:
        return _packed_strs(self.search_anchored_batch_packed([_utf8(s, 'substring')], anchor))

    def search_prefix(self, s: str) -> typing.List[str]:
        """Extension: the entries that start with ``s``."""
        return self._search_anchored_str(s, 'start')

    def search_suffix(self, s: str) -> typing.List[str]:
        """Extension: the entries that end with ``s``."""
        return self._search_anchored_str(s, 'end')

    def search_exact(self, s: str) -> typing.List[str]:
        """Extension: the entries equal to ``s`` (one per copy in the index)."""
        return self._search_anchored_str(s, 'entry')

    def has_entries(self, texts: typing.List[str]) -> typing.List[bool]:
        """Extension: for every text, whether the index holds an entry equal to it."""
        return [c > 0 for c in self.count_anchored_bytes([_utf8(t, 'text') for t in texts], 'entry')]

    @staticmethod
    def _terms_args(groups):
        """(blob, term offsets, group offsets, exclude flags) of one all-terms batch.  A group is an ``(include,
        exclude)`` pair of byte-string sequences, or a bare sequence of byte strings (no exclusions).  ``ValueError`` for
        a group without an include term and for an empty term."""
        import numpy as np
        terms: typing.List[bytes] = []
        flags: typing.List[int] = []
        goff = [0]
        for g, group in enumerate(groups):
            if isinstance(group, (bytes, bytearray, str)):
                raise TypeError(f'group {g} must be a sequence of byte strings or an (include, exclude) pair of them')
            group = list(group)
            if len(group) == 2 and not isinstance(group[0], (bytes, bytearray)) and not isinstance(group[1], (bytes, bytearray)):
                include, exclude = list(group[0]), list(group[1])
            else:
                include, exclude = group, []
            for t in include + exclude:
                if not isinstance(t, (bytes, bytearray)):
                    raise TypeError(f'group {g}: a term must be bytes, not {type(t).__name__}')
                if len(t) == 0:
                    raise ValueError(f'group {g}: an empty term (every entry contains it: leave it out)')
            if not include:
                raise ValueError(f'group {g} has no include term ("everything except" is not a search)')
            terms += [bytes(t) for t in include + exclude]
            flags += [0] * len(include) + [1] * len(exclude)
            goff.append(len(terms))
        blob, offs = _pack_queries(terms)
        return blob, offs, np.array(goff, dtype=np.uint64), np.array(flags if flags else [0], dtype=np.uint8)

    @_with_icase(_folded_batch('terms', 'packed'), _ICASE_ALL)
    def search_all_batch_packed(self, groups) -> 'PackedResult':
        """Extension: per group, the entries that contain EVERY include term and NO exclude term, as a packed result
        like ``search_batch_packed``'s with one row per group.  ``groups`` is a sequence of ``(include, exclude)``
        pairs of byte-string sequences; a bare sequence of byte strings means no exclusions.  "Contains" is what
        ``search`` means, so the answer is the intersection of the include terms' ``search_ids_batch`` results minus the
        union of the exclude terms'.  On the device the rarest include term of every (group, chunk) pair drives the
        search and its candidate entries are checked against the other terms, so the work follows the rarest term
        (include/pss.h).  ``set_result_order`` has no effect."""
        return self._group_batch('pss_reader_search_terms_batch', self._terms_args(groups), 'packed')

    @_with_icase(_folded_batch('terms', 'ids'), _ICASE_ALL)
    def search_all_ids_batch(self, groups) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_all_batch_packed`` returns, in the same
        order; ``counts[g]`` of them belong to group g."""
        return self._group_batch('pss_reader_search_terms_ids_batch', self._terms_args(groups), 'ids')

    @_with_icase(_folded_batch('terms', 'counts'), _ICASE_ALL)
    def count_all_bytes(self, groups) -> typing.List[int]:
        """Extension: how many entries each group matches; only the counters come back."""
        return self._group_batch('pss_reader_count_terms_batch', self._terms_args(groups), 'counts')

    @staticmethod
    def _str_terms(terms, exclude):
        if isinstance(terms, (str, bytes, bytearray)) or isinstance(exclude, (str, bytes, bytearray)):
            bad = terms if isinstance(terms, (str, bytes, bytearray)) else exclude
            raise TypeError(f"argument 'terms': '{type(bad).__name__}' object cannot be converted to a sequence of 'PyString'")
        return [([_utf8(t, 'terms') for t in terms], [_utf8(t, 'exclude') for t in exclude])]

    @_with_icase(_folded_search_all, _ICASE_ALL)
    def search_all(self, terms: typing.Sequence[str], exclude: typing.Sequence[str] = ()) -> typing.List[str]:
        """Extension: the entries that contain every one of ``terms`` and none of ``exclude``."""
        return _packed_strs(self.search_all_batch_packed(self._str_terms(terms, exclude)))

    @_with_icase(_folded_count_all, _ICASE_ALL)
    def count_all(self, terms: typing.Sequence[str], exclude: typing.Sequence[str] = ()) -> int:
        """Extension: how many entries contain every one of ``terms`` and none of ``exclude``."""
        return self.count_all_bytes(self._str_terms(terms, exclude))[0]

    @staticmethod
    def _glob_args(patterns):
        """(blob, segment offsets, group offsets, anchor bytes) of one batch of glob patterns (``glob_parse`` of each)."""
        import numpy as np
        if isinstance(patterns, (bytes, bytearray, str)):
            raise TypeError(f"argument 'patterns': '{type(patterns).__name__}' object cannot be converted to a sequence of glob patterns")
        segs: typing.List[bytes] = []
        goff = [0]
        anch: typing.List[int] = []
        for g, pat in enumerate(patterns):
            if not isinstance(pat, (bytes, bytearray)):
                raise TypeError(f'pattern {g}: a glob pattern must be bytes, not {type(pat).__name__}')
            parts, a = glob_parse(pat)
            segs += parts
            goff.append(len(segs))
            anch.append(a)
        blob, offs = _pack_queries(segs)
        return blob, offs, np.array(goff, dtype=np.uint64), np.array(anch if anch else [0], dtype=np.uint8)

    @_with_icase(_folded_batch('seq', 'packed'), _ICASE_GLOB, _classed_batch('packed'))
    def search_glob_batch_packed(self, patterns: typing.Sequence[bytes]) -> 'PackedResult':
        """Extension: per glob pattern (``glob_parse``: literal pieces and ``*``), the entries that hold the pieces IN
        ORDER and without overlap -- the first at the entry's start unless the pattern begins with ``*``, the last at its
        end unless it ends with one -- as a packed result like ``search_batch_packed``'s with one row per pattern.  Exact
        bytes; every entry at most once per pattern; a piece holding a newline matches nothing.  On the device the rarest
        piece of every (pattern, chunk) pair drives the search and each candidate entry is walked once, left to right
        (include/pss.h, pss_reader_search_seq_batch).  ``set_result_order`` has no effect."""
        return self._group_batch('pss_reader_search_seq_batch', self._glob_args(patterns), 'packed')

    @_with_icase(_folded_batch('seq', 'ids'), _ICASE_GLOB, _classed_batch('ids'))
    def search_glob_ids_batch(self, patterns: typing.Sequence[bytes]) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_glob_batch_packed`` returns, in the same
        order; ``counts[g]`` of them belong to pattern g."""
        return self._group_batch('pss_reader_search_seq_ids_batch', self._glob_args(patterns), 'ids')

    @_with_icase(_folded_batch('seq', 'counts'), _ICASE_GLOB, _classed_batch('counts'))
    def count_glob_bytes(self, patterns: typing.Sequence[bytes]) -> typing.List[int]:
        """Extension: how many entries each glob pattern matches; only the counters come back."""
        return self._group_batch('pss_reader_count_seq_batch', self._glob_args(patterns), 'counts')

    @_with_icase(_folded_search_glob, _ICASE_GLOB, _classed_search_glob)
    def search_glob(self, s: str) -> typing.List[str]:
        """Extension: the entries that match the glob pattern ``s`` (``*`` = any run of bytes, ``\\`` escapes)."""
        return _packed_strs(self.search_glob_batch_packed([_utf8(s, 'pattern')]))

    @_with_icase(_folded_count_glob, _ICASE_GLOB, _classed_count_glob)
    def count_glob(self, s: str) -> int:
        """Extension: how many entries match the glob pattern ``s``."""
        return self.count_glob_bytes([_utf8(s, 'pattern')])[0]

    def _regex_batch(self, form: str, patterns, icase):
        """One ``pss_reader_search_regex_*`` call over ``patterns`` (each ``bytes``, or ``str`` UTF-8 encoded)."""
        flags = _ffi.REGEX_ICASE if _icase_flag(icase) else 0
        if isinstance(patterns, (bytes, bytearray, str)):
            raise TypeError(f"argument 'patterns': '{type(patterns).__name__}' object cannot be converted to a sequence of regex patterns")
        blob, offs = _pack_queries([_regex_bytes(p) for p in patterns])
        name = {'packed': 'pss_reader_search_regex_batch', 'ids': 'pss_reader_search_regex_ids_batch',
                'counts': 'pss_reader_count_regex_batch'}[form]
        np_ = len(offs) - 1
        return self._batch(getattr(_lib, name), (blob, offs.ctypes.data, np_, flags), np_, form)

    def search_regex_batch_packed(self, patterns: typing.Sequence[bytes], *, icase: bool = False) -> 'PackedResult':
        """Extension: per regular expression, the entries ``e`` with ``re.search(pattern, e, re.I if icase else 0)`` as a
        packed result like ``search_batch_packed``'s with one row per pattern.  The syntax is a subset of ``re`` over bytes:
        literals, ``.``, escapes, ``\\d \\w \\s`` and their complements, sets, groups, ``|``, ``* + ? {m,n}``, ``^`` as the first
        and ``$`` as the last byte (the entry's two ends); lazy and possessive quantifiers, back-references, look-around,
        ``\\b``, inline flags and named groups are a ``ValueError`` that names the position, and so is a pattern without a
        REQUIRED LITERAL (``regex_literals``): the literals are looked up as an all-terms group, the rarest per (pattern,
        chunk) drives, and every candidate entry is walked once through the pattern's DFA on the device (``regex_info``;
        include/pss.h, pss_reader_search_regex_batch).  A ``str`` pattern is UTF-8 encoded; ``icase`` folds ``A-Z`` / ``a-z``
        only.  A literal holding a newline matches nothing.  Always the general pipeline; ``set_result_order`` has no
        effect."""
        return self._regex_batch('packed', patterns, icase)

    def search_regex_ids_batch(self, patterns: typing.Sequence[bytes], *, icase: bool = False) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_regex_batch_packed`` returns, in the same
        order; ``counts[g]`` of them belong to pattern g."""
        return self._regex_batch('ids', patterns, icase)

    def count_regex_bytes(self, patterns: typing.Sequence[bytes], *, icase: bool = False) -> typing.List[int]:
        """Extension: how many entries each regular expression matches; only the counters come back."""
        return self._regex_batch('counts', patterns, icase)

    def search_regex(self, s: str, *, icase: bool = False) -> typing.List[str]:
        """Extension: the entries that match the regular expression ``s`` (``search_regex_batch_packed``)."""
        return _packed_strs(self.search_regex_batch_packed([s], icase=icase))

    def count_regex(self, s: str, *, icase: bool = False) -> int:
        """Extension: how many entries match the regular expression ``s``."""
        return self.count_regex_bytes([s], icase=icase)[0]

    def _any_batch(self, form: str, sets, icase):
        """One ``pss_reader_search_any_*`` call over ``sets``, a sequence of sequences of ``bytes``."""
        import numpy as np
        flags = _ffi.ANY_ICASE if _icase_flag(icase) else 0
        if isinstance(sets, (bytes, bytearray, str)):
            raise TypeError(f"argument 'sets': '{type(sets).__name__}' object cannot be converted to a sequence of sets")
        alts: typing.List[bytes] = []
        soff = [0]
        for g, one in enumerate(sets):
            alts += _any_set(one, f'set {g}')
            soff.append(len(alts))
        blob, offs = _pack_queries(alts)
        soff = np.array(soff, dtype=np.uint64)
        name = {'packed': 'pss_reader_search_any_batch', 'ids': 'pss_reader_search_any_ids_batch',
                'counts': 'pss_reader_count_any_batch'}[form]
        ns = len(soff) - 1
        return self._batch(getattr(_lib, name), (blob, offs.ctypes.data, len(alts), soff.ctypes.data, ns, flags), ns, form)

    def search_any_batch_packed(self, sets: typing.Sequence[typing.Sequence[bytes]], *, icase: bool = False) -> 'PackedResult':
        """Extension: per SET of alternatives, the entries that contain AT LEAST ONE of them (``grep -e a -e b``), as a
        packed result like ``search_batch_packed``'s with one row per set.  "Contains" is what ``search`` means -- exact
        bytes -- or, with ``icase=True``, what ``search_icase`` means: only ``A-Z`` / ``a-z`` fold.  Every entry comes at
        most once per set.  The set is normalised on the host (``any_alternatives``: duplicates, alternatives with a
        newline and alternatives that hold another one go; at most 64 are left, 32 under ``icase``, else ``ValueError``),
        its alternatives -- under ``icase`` the spellings of their seeds -- are looked up as the queries of one term, and
        the device keeps the hit of every entry's leftmost match (include/pss.h, pss_reader_search_any_batch).  A set
        whose alternatives all hold a newline matches nothing.  Inside a (set, chunk) pair the entries come by alternative
        (ascending), then spelling, then in suffix-array order: a set of one alternative returns what ``search_ids_batch``
        (``icase``: ``search_icase_ids_batch``) returns, order included.  Always the general pipeline;
        ``set_result_order`` has no effect.  ``ValueError`` for an empty set or alternative, ``TypeError`` for a member
        that is not ``bytes`` and an ``icase`` that is not a bool."""
        return self._any_batch('packed', sets, icase)

    def search_any_ids_batch(self, sets: typing.Sequence[typing.Sequence[bytes]], *, icase: bool = False) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_any_batch_packed`` returns, in the same
        order; ``counts[g]`` of them belong to set g."""
        return self._any_batch('ids', sets, icase)

    def count_any_bytes(self, sets: typing.Sequence[typing.Sequence[bytes]], *, icase: bool = False) -> typing.List[int]:
        """Extension: how many entries each set matches; only the counters come back."""
        return self._any_batch('counts', sets, icase)

    @staticmethod
    def _str_any(terms):
        if isinstance(terms, (str, bytes, bytearray)):
            raise TypeError(f"argument 'terms': '{type(terms).__name__}' object cannot be converted to a sequence of 'PyString'")
        return [[_utf8(t, 'terms') for t in terms]]

    def search_any(self, terms: typing.Sequence[str], *, icase: bool = False) -> typing.List[str]:
        """Extension: the entries that contain at least one of ``terms`` (``search_any_batch_packed``); with
        ``icase=True`` whatever the case of ASCII letters."""
        return _packed_strs(self.search_any_batch_packed(self._str_any(terms), icase=icase))

    def count_any(self, terms: typing.Sequence[str], *, icase: bool = False) -> int:
        """Extension: how many entries contain at least one of ``terms``."""
        return self.count_any_bytes(self._str_any(terms), icase=icase)[0]

    @staticmethod
    def _icase_args(patterns):
        """(blob, offsets) of one batch of case-insensitive patterns; ``ValueError`` for an empty pattern."""
        if isinstance(patterns, (bytes, bytearray, str)):
            raise TypeError(f"argument 'patterns': '{type(patterns).__name__}' object cannot be converted to a sequence of patterns")
        patterns = list(patterns)
        for q, pat in enumerate(patterns):
            if not isinstance(pat, (bytes, bytearray)):
                raise TypeError(f'pattern {q}: a pattern must be bytes, not {type(pat).__name__}')
            if len(pat) == 0:
                raise ValueError(f'pattern {q} is empty (every entry contains the empty pattern)')
        return _pack_queries([bytes(p) for p in patterns])

    def search_icase_batch_packed(self, patterns: typing.Sequence[bytes]) -> 'PackedResult':
        """Extension: per pattern, the entries that contain it whatever the case of its ASCII letters (``grep -i``), as a
        packed result like ``search_batch_packed``'s.  Only the ASCII letters ``A-Z`` / ``a-z`` fold: every other byte,
        ``0x80 .. 0xFF`` included (so every letter outside ASCII), matches only itself.  Every entry at most once per
        pattern; a pattern holding a newline matches nothing; an empty pattern is a ``ValueError``.  The suffix arrays are
        exact-byte: the spellings of a SEED of the pattern (``icase_variants``) are looked up and every hit is verified
        against the whole pattern on the device, so the work follows the occurrences of the folded seed
        (include/pss.h, pss_reader_search_icase_batch).  ``set_result_order`` has no effect."""
        return self._query_batch('pss_reader_search_icase_batch', self._icase_args(patterns), 'packed')

    def search_icase_ids_batch(self, patterns: typing.Sequence[bytes]) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_icase_batch_packed`` returns, in the same
        order; ``counts[q]`` of them belong to pattern q.  Only ASCII letters fold.  A pattern without an ASCII letter
        returns exactly what ``search_ids_batch`` returns for it."""
        return self._query_batch('pss_reader_search_icase_ids_batch', self._icase_args(patterns), 'ids')

    def count_icase_bytes(self, patterns: typing.Sequence[bytes]) -> typing.List[int]:
        """Extension: how many entries contain each pattern whatever the case of its ASCII letters (only they fold); only
        the counters come back."""
        return self._query_batch('pss_reader_count_icase_batch', self._icase_args(patterns), 'counts')

    def search_icase(self, s: str) -> typing.List[str]:
        """Extension: the entries that contain ``s`` (UTF-8 encoded) whatever the case of its ASCII letters.  Only
        ``A-Z`` / ``a-z`` fold: ``'é'`` does not match ``'É'``."""
        return _packed_strs(self.search_icase_batch_packed([_utf8(s, 'substring')]))

    def count_icase(self, s: str) -> int:
        """Extension: how many entries contain ``s`` (UTF-8 encoded) whatever the case of its ASCII letters (only they
        fold)."""
        return self.count_icase_bytes([_utf8(s, 'substring')])[0]

    @staticmethod
    def _near_args(patterns, k, edits=False, icase=False):
        """(blob, offsets, budgets) of one batch within k mismatches, or within k edits (``edits``, a bool), in exact bytes or
        under ASCII case folding (``icase``, a bool: the checks are the same).  ``k`` is an int
        for the batch or a sequence with one int per pattern; ``ValueError`` for an empty pattern, a budget outside 0 .. 3,
        a pattern of at most its budget's bytes, or another number of budgets than patterns."""
        import numpy as np
        if not isinstance(edits, bool):
            raise TypeError(f"argument 'edits' must be a bool, not {type(edits).__name__}")
        if not isinstance(icase, bool):
            raise TypeError(f"argument 'icase' must be a bool, not {type(icase).__name__}")
        if isinstance(patterns, (bytes, bytearray, str)):
            raise TypeError(f"argument 'patterns': '{type(patterns).__name__}' object cannot be converted to a sequence of patterns")
        patterns = list(patterns)
        if isinstance(k, (bytes, bytearray, str)):
            raise TypeError(f'a mismatch budget k must be an int (or one per pattern), not {type(k).__name__}')
        if not hasattr(k, '__iter__'):
            budgets = [_near_budget(k)] * len(patterns)
        else:
            budgets = [_near_budget(b) for b in k]
            if len(budgets) != len(patterns):
                raise ValueError(f'{len(budgets)} budgets for {len(patterns)} patterns')
        for q, (pat, b) in enumerate(zip(patterns, budgets)):
            if not isinstance(pat, (bytes, bytearray)):
                raise TypeError(f'pattern {q}: a pattern must be bytes, not {type(pat).__name__}')
            if len(pat) == 0:
                raise ValueError(f'pattern {q} is empty (every entry contains the empty pattern)')
            if len(pat) <= b and edits:
                raise ValueError(f'pattern {q} has {len(pat)} bytes and a budget of {b} edits: deleting all of it matches every entry')
            if len(pat) <= b:
                raise ValueError(f'pattern {q} has {len(pat)} bytes and a budget of {b} mismatches: every window of its length matches it')
        blob, offs = _pack_queries([bytes(p) for p in patterns])
        return blob, offs, np.array(budgets, dtype=np.uint8)

    def _near_batch(self, form: str, patterns, k, edits, icase):
        """One batch within k through the C call of its kind: near, edit, or -- ``icase`` -- either under fold."""
        blob, offs, ks = self._near_args(patterns, k, edits, icase)
        if not icase:
            name = {'packed': 'pss_reader_search_%s_batch', 'ids': 'pss_reader_search_%s_ids_batch', 'counts': 'pss_reader_count_%s_batch'}[form]
            return self._query_batch(name % ('edit' if edits else 'near'), (blob, offs), form, ks)
        name = {'packed': 'pss_reader_search_near_icase_batch', 'ids': 'pss_reader_search_near_icase_ids_batch',
                'counts': 'pss_reader_count_near_icase_batch'}[form]
        nq = len(offs) - 1
        return self._batch(getattr(_lib, name), (blob, offs.ctypes.data, nq, ks.ctypes.data, int(edits)), nq, form)

    def search_near_batch_packed(self, patterns: typing.Sequence[bytes], k=1, edits: bool = False, *, icase: bool = False) -> 'PackedResult':
        """Extension: per pattern, the entries that hold it with at most ``k`` bytes SUBSTITUTED (Hamming distance:
        ``passw0rd`` for ``password`` at ``k=1``), as a packed result like ``search_batch_packed``'s.  ``k`` is 0 .. 3, one
        int for the batch or a sequence with one per pattern.  The window lies inside the entry; bytes are exact (nothing
        folds); every entry at most once per pattern; a pattern holding a newline matches nothing.  ``ValueError`` for an
        empty pattern, ``k > 3`` and a pattern of at most ``k`` bytes.  No insertions or deletions.  The pattern's ``k + 1``
        pieces (``near_pieces``) are looked up and every hit is verified on the device, so the work follows the
        occurrences of the pieces (include/pss.h, pss_reader_search_near_batch).  ``set_result_order`` has no effect.

        ``edits=True``: the budget counts EDITS -- bytes inserted, deleted or substituted (Levenshtein distance over bytes:
        ``pasword``, ``passsword`` and ``passw0rd`` for ``password`` at ``k=1``).  An entry matches iff some substring of it
        is within ``k`` edits of the pattern; the substring lies inside the entry.  Everything else as above: the same
        pieces, every occurrence of a piece verified on the device (include/pss.h, pss_reader_search_edit_batch).  The
        answer contains the answer without ``edits`` at the same ``k``.

        ``icase=True`` (keyword only; combines with ``edits``): two bytes are equal iff they are equal after folding ``A-Z``
        to ``a-z`` -- the rule of ``search_icase_batch_packed``; nothing else folds, ``0x80 .. 0xFF`` match only themselves.
        A case difference costs nothing: ``passw0rd`` and ``PASSW0RD`` for ``Password`` at ``k=1``.  Everything else as above.
        Each piece is looked up through the spellings of its seed (``near_seeds``), at most 64 queries per pattern, and
        every hit is verified under fold on the device (include/pss.h, pss_reader_search_near_icase_batch).  ``k=0`` returns
        exactly what ``search_icase_ids_batch`` returns; for every ``k`` the answer contains the answer without ``icase``."""
        return self._near_batch('packed', patterns, k, edits, icase)

    def search_near_ids_batch(self, patterns: typing.Sequence[bytes], k=1, edits: bool = False, *, icase: bool = False) -> 'IdResult':
        """Extension: the ids (``search_ids_batch``) of the entries ``search_near_batch_packed`` returns, in the same
        order; ``counts[q]`` of them belong to pattern q.  ``k=0`` returns exactly what ``search_ids_batch`` returns.
        ``edits=True``: the entries within ``k`` edits instead (``search_near_batch_packed``); ``k=0`` is the same.
        ``icase=True``: under ASCII case folding (``search_near_batch_packed``); ``k=0`` returns exactly what
        ``search_icase_ids_batch`` returns."""
        return self._near_batch('ids', patterns, k, edits, icase)

    def count_near_bytes(self, patterns: typing.Sequence[bytes], k=1, edits: bool = False, *, icase: bool = False) -> typing.List[int]:
        """Extension: how many entries hold each pattern within ``k`` mismatches (``edits=True``: within ``k`` edits;
        ``icase=True``: under ASCII case folding); only the counters come back."""
        return self._near_batch('counts', patterns, k, edits, icase)

    def search_near(self, s: str, k: int = 1, edits: bool = False, *, icase: bool = False) -> typing.List[str]:
        """Extension: the entries that hold ``s`` (UTF-8 encoded) with at most ``k`` BYTES substituted -- with
        ``edits=True``: inserted, deleted or substituted; with ``icase=True``: whatever the case of ASCII letters."""
        return _packed_strs(self.search_near_batch_packed([_utf8(s, 'substring')], _near_budget(k), edits, icase=icase))

    def count_near(self, s: str, k: int = 1, edits: bool = False, *, icase: bool = False) -> int:
        """Extension: how many entries hold ``s`` (UTF-8 encoded) with at most ``k`` bytes substituted -- with
        ``edits=True``: inserted, deleted or substituted; with ``icase=True``: whatever the case of ASCII letters."""
        return self.count_near_bytes([_utf8(s, 'substring')], _near_budget(k), edits, icase=icase)[0]

    @staticmethod
    def _span_ids(ids, counts, npatterns: int):
        """(ids as uint64, id offsets as uint64) of one span batch; ``ValueError`` when ``counts`` has another length than
        the patterns or another sum than ``ids`` has entries."""
        import numpy as np
        arr = np.ascontiguousarray(np.asarray(ids).reshape(-1) if len(ids) else np.zeros(0, dtype=np.uint64))
        if arr.dtype != np.uint64:
            if arr.dtype.kind not in 'iu':
                raise TypeError('entry ids must be integers')
            if arr.dtype.kind == 'i' and arr.size and int(arr.min()) < 0:
                raise ValueError('entry ids are not negative')
            arr = arr.astype(np.uint64)
        cnt = np.asarray(counts).reshape(-1) if len(counts) else np.zeros(0, dtype=np.uint64)
        if cnt.dtype.kind not in 'iu':
            raise TypeError('counts must be integers')
        if cnt.dtype.kind == 'i' and cnt.size and int(cnt.min()) < 0:
            raise ValueError('counts are not negative')
        if cnt.size != npatterns:
            raise ValueError(f'{cnt.size} counts for {npatterns} patterns')
        offs = np.zeros(npatterns + 1, dtype=np.uint64)
        np.cumsum(cnt.astype(np.uint64), out=offs[1:])
        if int(offs[-1]) != arr.size:
            raise ValueError(f'the counts add up to {int(offs[-1])} rows, ids has {arr.size}')
        return arr, offs

    def match_spans_batch(self, ids, counts, patterns: typing.Sequence[bytes], k=1, edits: bool = False, *, icase: bool = False):
        """Extension: WHERE and HOW CLOSELY entries match -- for the ids and counts of an ``IdResult`` (``counts[q]`` ids
        in a row belong to pattern q; any ids will do, repeated or of several chunks) the best match of each entry's pattern
        as a numpy int32 array ``[len(ids), 3]`` with the columns ``start, length, distance``, row i answering ``ids[i]``.
        ``patterns``, ``k``, ``edits`` and ``icase`` are ``search_near_ids_batch``'s, argument for argument, with the same
        checks: the call that explains an answer takes what the call that found it took.

        A candidate is a substring of the entry: without ``edits`` a window of ``len(pattern)`` bytes, its distance the
        number of differing bytes; with ``edits`` any non-empty substring, its distance the Levenshtein distance over bytes
        (``icase``: bytes equal after folding ``A-Z`` to ``a-z`` cost nothing).  Among the candidates within ``k`` the row is
        the CLOSEST, then the leftmost, then the longest -- ``passw0rd password`` is highlighted at ``password``.  An entry
        with no candidate within ``k`` is ``(-1, 0, -1)``, and so is every row of a pattern that holds a newline; hence
        ``distance >= 0`` exactly for the ids ``search_near_ids_batch`` returns, and ``length == len(pattern)`` without
        ``edits``.  Offsets count BYTES from the entry's first byte: slice the entry's bytes,
        ``entry_bytes[start:start + length]``, not its decoded text, where entries hold UTF-8.
        ``ValueError`` when ``sum(counts) != len(ids)`` or ``len(counts) != len(patterns)``, and for an id of a chunk this
        reader does not hold or a line its chunk does not have (``entries_by_id``).  The scan runs on the device, one
        wavefront per row; 12 bytes per row come down and no text (include/pss.h, pss_reader_match_spans)."""
        import numpy as np
        blob, offs, ks = self._near_args(patterns, k, edits, icase)
        nq = len(offs) - 1
        arr, id_offs = self._span_ids(ids, counts, nq)
        out = np.empty((arr.size, 3), dtype=np.int32)
        flags = (_ffi.SPAN_EDITS if edits else 0) | (_ffi.SPAN_ICASE if icase else 0)
        _ffi.check(_lib.pss_reader_match_spans(self._handle(), arr.ctypes.data, id_offs.ctypes.data, blob, offs.ctypes.data, nq,
                                               ks.ctypes.data, flags, out.ctypes.data))
        return out

    def match_spans(self, ids, pattern, k: int = 1, edits: bool = False, *, icase: bool = False):
        """Extension: ``match_spans_batch`` for ONE pattern (bytes, or a str that is UTF-8 encoded) and the ids it is asked
        about: int32 ``[len(ids), 3]``, columns ``start, length, distance`` in bytes."""
        pat = pattern.encode('utf-8') if isinstance(pattern, str) else pattern
        return self.match_spans_batch(ids, [len(ids)], [pat], _near_budget(k), edits, icase=icase)

    @property
    def entry_counts(self) -> typing.Dict[int, int]:
        """Extension: entries of every chunk this reader holds, keyed by the chunk's index in the index file."""
        num = ctypes.c_uint64()
        _ffi.check(_lib.pss_reader_chunk_entries(self._handle(), None, None, 0, ctypes.byref(num)))
        k = int(num.value)
        idx = (ctypes.c_uint64 * max(k, 1))()
        ent = (ctypes.c_uint64 * max(k, 1))()
        _ffi.check(_lib.pss_reader_chunk_entries(self._handle(), idx, ent, k, ctypes.byref(num)))
        return {int(idx[i]): int(ent[i]) for i in range(min(k, int(num.value)))}

    def entry_ordinals(self, ids):
        """Extension: ids -> 0-based positions of the entries in the order they were added (numpy int64): entries of
        the chunks before the id's chunk, plus its line.  For an index made by one ``add_entries_from_file_lines``
        call that is the line number in the source file.  ``ValueError`` when this reader does not hold every chunk
        of the file from 0 up to the largest one named (a shard cannot know what the others hold)."""
        import numpy as np
        arr = np.asarray(ids, dtype=np.uint64).reshape(-1)
        if not arr.size:
            return np.zeros(0, dtype=np.int64)
        chunk = (arr >> np.uint64(32)).astype(np.int64)
        line = (arr & np.uint64(0xffffffff)).astype(np.int64)
        counts = self.entry_counts
        top = int(chunk.max())
        missing = [c for c in range(top + 1) if c not in counts]
        if missing:
            raise ValueError(f'entry_ordinals needs every chunk from 0 to {top}; this reader does not hold chunk {missing[0]}')
        per = np.array([counts[c] for c in range(top + 1)], dtype=np.int64)
        if (line >= per[chunk]).any():
            bad = int(arr[np.argmax(line >= per[chunk])])
            raise ValueError(f'entry id {bad:#x}: chunk {bad >> 32} has {int(per[bad >> 32])} entries')
        base = np.concatenate(([0], np.cumsum(per)[:-1]))
        return base[chunk] + line

    def search_batch_device(self, patterns: typing.Sequence[bytes]) -> 'DeviceResult':
        """One batched device call whose packed result STAYS in HBM (torch tensors, no copy): what the
        multi-GPU gather sends over RCCL (``dist.gather_device``).  Needs torch."""
        import numpy as np
        import torch
        nq = len(patterns)
        blob, offs = _pack_queries(patterns)
        dr = _ffi.DeviceResult()
        _ffi.check(_lib.pss_reader_search_batch_device(self._handle(), blob, offs.ctypes.data, nq, ctypes.byref(dr)))
        dev = torch.device('cuda', dr.device)

        def wrap(ptr, nbytes, dtype):
            if not nbytes or not ptr:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_DevicePtr(ptr, nbytes), device=dev).view(dtype)

        # The three ranges are slots of the device's shared workspace: another handle or thread on the device may
        # reuse them as soon as the call has returned.  Own them before anyone else gets in (device-to-device, a few
        # microseconds for the sizes a batch produces).
        out = DeviceResult(wrap(dr.d_bytes, dr.num_bytes, torch.uint8).clone(), wrap(dr.d_offsets, dr.num_entries * 8, torch.int64).clone(),
                           wrap(dr.d_counts, nq * 8, torch.int64).clone(), int(dr.num_bytes))
        torch.cuda.current_stream(dev).synchronize()
        return out

    def search_multiple_bytes_as_str(self, patterns: typing.Sequence[bytes]) -> typing.List[str]:
        """``search_multiple`` for queries that are already UTF-8 bytes."""
        return self._search_batch(patterns, True)[0]

    def count_multiple_bytes(self, patterns: typing.Sequence[bytes]) -> typing.List[int]:
        """``count_multiple`` for queries that are already bytes."""
        return self._query_batch('pss_reader_count_batch', _pack_queries(patterns), 'counts')

    def search_batch_raw(self, patterns: typing.Sequence[bytes]):
        """One batched device call.  Returns (entries, per_query_counts): the
        entry byte strings query-major, and how many belong to each query."""
        return self._search_batch(patterns, False)

    def last_stats(self) -> dict:
        """Statistics of the last batch (pss_search_stats): counts, times, and ``route`` -- the PSS_ROUTE_* bits of
        the search routes that served it (``_ffi.ROUTES`` names them)."""
        st = _ffi.SearchStats()
        _ffi.check(_lib.pss_reader_last_stats(self._handle(), ctypes.byref(st)))
        return st.as_dict()

    def search(self, substring: str) -> typing.List[str]:
        return self._search_batch([_utf8(substring, 'substring')], True)[0]

    def search_multiple(self, substrings: typing.List[str]) -> typing.List[str]:
        return self._search_batch([_utf8(s, 'substring') for s in substrings], True)[0]

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            _lib.pss_reader_close(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
