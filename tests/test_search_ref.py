"""CPU tests of tests/search_ref.py, the suffix-array-free restatement of Reader::search that
tests/test_search_edges_gpu.py compares every search route with: against the reference's own tests as data and
against the oracle's search (oracle/pss_oracle.c) on random indexes."""
import json
import os
import pathlib
import random

from tests.search_ref import SearchRef

HERE = os.path.dirname(os.path.abspath(__file__))


def build_idx(W, path, entries):
    w = W(path)
    for e in entries:
        w.add_entry(e)
    w.finalize()
    w.close()


def test_reference_tests_as_data(oracle, tmp_path):
    oracle.use_reference_sa(False)
    cases = json.loads(pathlib.Path(HERE, 'golden', 'reference_cases.json').read_text(encoding='utf-8'))['cases']
    for case in cases:
        if 'missing_path' in case:
            continue
        p = str(tmp_path / (case['name'] + '.idx'))
        build_idx(oracle.OracleWriter, p, case['entries'])
        ref = SearchRef.from_index(p)
        for s in case['searches']:
            got = [e.decode('utf-8') for e in ref.search(s['substring'].encode('utf-8'))]
            assert sorted(got) == sorted(s['expected']), (case['name'], s['substring'])
        for s in case['search_multiple']:
            ents, _ = ref.search_multiple([q.encode('utf-8') for q in s['substrings']])
            assert sorted(e.decode('utf-8') for e in ents) == sorted(s['expected']), case['name']


def test_random_indexes_against_the_oracle(oracle, tmp_path):
    """Empty entries, 0x00 / 0xFF bytes, queries with '\\n', several chunks: counts and per-query multisets."""
    oracle.use_reference_sa(False)
    rng = random.Random(17)
    for k in range(8):
        alphabet = rng.choice([b'ab\x00\xff', b'a\n\x00', b'\x00\xff\n\x7f\x80', b'abc\n\n'])
        n = rng.choice([40, 400, 3000])
        data = bytes(rng.choice(alphabet) for _ in range(n))
        src = tmp_path / f'r{k}.txt'
        src.write_bytes(data + (b'\n' if k % 2 else b''))
        p = str(tmp_path / f'r{k}.idx')
        w = oracle.OracleWriter(p, rng.choice([None, 64, 300]))
        w.add_entries_from_file_lines(str(src))
        w.finalize()
        w.close()
        queries = [b'', b'\n', b'\x00', b'\xff', b'\x00\n', b'\n\x00', b'zz', b'\x00' * 9]
        for _ in range(60):
            s = rng.randrange(len(data))
            queries.append(data[s:s + rng.randint(1, 12)])
        ref = SearchRef.from_index(p)
        ents, counts = ref.search_multiple(queries)
        r = oracle.OracleReader(p)
        oe, oc = r.search_multiple_bytes(queries)
        assert r.num_chunks == len(ref.chunks)
        r.close()
        assert counts == oc.tolist(), k
        for q in queries[:12]:                     # hits per chunk: every start position, overlapping ones included
            assert ref.hits(q) == [sum(ch.text.startswith(q, i) for i in range(len(ch.text))) for ch in ref.chunks], q
        pos = 0
        for c in counts:
            assert sorted(ents[pos:pos + c]) == sorted(oe[pos:pos + c]), k
            pos += c
