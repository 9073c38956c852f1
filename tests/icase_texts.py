"""Texts of the case-insensitive suites (tests/test_icase_gpu.py, tests/test_icase_groups_gpu.py): bytes with the case of
their letters flipped at random, and the byte pairs that differ by 0x20 and do not fold."""
import numpy as np

from tests.search_harness import filler

PAIRS_0X20 = ((b'@', b'`'), (b'[', b'{'), (b'\\', b'|'), (b'\xc1', b'\xe1'), (b'\x00', b' '), (b']', b'}'), (b'^', b'~'), (b'\xd0', b'\xf0'))


def mangle(rng, b, p=0.5):
    """b with the case of its ASCII letters flipped at random."""
    a = np.frombuffer(bytes(b), np.uint8).copy()
    letter = ((a | 0x20) >= 0x61) & ((a | 0x20) <= 0x7A)
    a[letter & (rng.random(a.size) < p)] ^= 0x20
    return a.tobytes()


def mixed_case_lines(rng, n, lo=0, hi=24):
    return [mangle(rng, filler(rng, int(rng.integers(lo, hi))), 0.3) for _ in range(n)]
