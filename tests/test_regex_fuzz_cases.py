"""Self-check of the generator of tests/regex_fuzz_cases.py on the reference alone (Python's re and the required literals):
every drawn pattern compiles -- the generator stays inside the subset, no case is left out --, at least half the rows have a
non-empty answer, and at least a quarter have a candidate that holds every literal and fails the expression: the rows that
show the verify kernel at work.  CPU only."""
import re
import warnings

from pysubstringsearch_amd import regex_info, regex_literals
from tests.regex_fuzz_cases import PER_BATCH, SEEDS, make_regex_case


def test_the_generator_is_a_function_of_the_seed():
    a, b = make_regex_case(3), make_regex_case(3)
    assert a == b and a.regex != make_regex_case(4).regex
    assert len(a.regex) == len(a.regex_icase) == PER_BATCH and len(a.pairs) == 8 * PER_BATCH


def test_every_pattern_compiles_and_the_rows_are_worth_running():
    rows = answered = near = 0
    kinds = set()
    for seed in SEEDS:
        case = make_regex_case(seed)
        entries = case.base.entries
        assert all(b'\n' not in s for _, s, _ in case.pairs)
        for batch, fold in ((case.regex, False), (case.regex_icase, True)):
            for pat in batch:
                with warnings.catch_warnings():
                    warnings.simplefilter('error')
                    rx = re.compile(pat, re.I if fold else 0)
                lits = regex_literals(pat, fold)                      # (a ValueError here: the generator left the subset)
                assert lits and regex_info(pat, fold)['states'] <= 4096
                held = [e.lower() if fold else e for e in entries]
                match = [rx.search(e) is not None for e in entries]
                assert all(all(lit in h for lit in lits) for h, m in zip(held, match) if m), pat     # the literals are sound
                rows += 1
                answered += any(match)
                near += any(not m and all(lit in h for lit in lits) for h, m in zip(held, match))
                kinds |= {k for k in (b'^', b'$', b'|', b'(?:', b'[^', b'{', b'\\w', b'.*', b'+') if k in pat}
    assert rows == 2 * PER_BATCH * len(SEEDS)
    assert 2 * answered >= rows, (answered, rows)
    assert 4 * near >= rows, (near, rows)
    assert len(kinds) == 9
