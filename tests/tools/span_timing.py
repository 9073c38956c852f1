"""Match spans next to the search whose answer they explain and next to the route a user had before them, on the same
patterns (MI355X; run by hand, not by the suite):

    python tests/tools/span_timing.py [--commit HASH] [--out profiles/match_spans_vs_host.json]

One 64 MiB chunk of `words` text (pss_gen_corpus, closed with a newline), its suffix array by pss_sa_build, handed to a
reader on the device.  32 patterns of 8 .. 12 letters, words of the text spread over its frequency ranking (the patterns of
tests/tools/near_timing.py and edit_timing.py), every budget k = 1.  For each of the four combinations of edits x icase, on
the same reader:
    near          search_near_ids_batch(patterns, 1, edits, icase=icase) alone: the call whose answer is being explained;
    spans_page    match_spans_batch on a page of that answer -- its first `--page` ids (2 000), with their patterns;
    spans_all     match_spans_batch on the whole answer;
    host_page     the route before: entries_by_id_packed of the page's ids, then per row the scoring of tests/span_ref.py
                  (numpy over the starts of one entry) in Python.
Before anything is timed host_page's rows are compared with spans_page's.  Each leg is warmed up, then timed with a host
clock around the whole leg (every library call ends in a stream synchronise); the legs alternate for `--rounds` rounds.  The
device legs run `--reps` times a round, host_page three times after one warm-up (a call takes seconds).  Reported:
median / min / max per leg and round.  Not measured here: k = 3, long entries, several chunks.  No threshold: a record, not
a test."""
import json
import statistics

import numpy as np

from timing_common import arguments, commit_hash, medians, pick_patterns, time_legs, words_reader, write_json

from tests.span_ref import span


def first_rows(res, rows):
    """(ids, counts) of the first `rows` ids of an IdResult, each with its pattern."""
    left, counts = rows, []
    for c in res.counts.tolist():
        counts.append(min(int(c), left))
        left -= counts[-1]
    return res.ids[:sum(counts)], counts


def main():
    ap_args = arguments('match_spans_vs_host.json', ('--page', 2000))
    host_reps = 3
    r, text, _ = words_reader()
    patterns = pick_patterns(text.tobytes(), 32)
    runs, summary, answers = [], {}, {}
    for edits in (False, True):
        for icase in (False, True):
            tag = ('edit' if edits else 'near') + ('_icase' if icase else '')
            res = r.search_near_ids_batch(patterns, 1, edits=edits, icase=icase)
            all_ids, all_counts = res.ids.copy(), res.counts.tolist()
            page_ids, page_counts = first_rows(res, ap_args.page)
            page_ids = page_ids.copy()
            pat_of = np.repeat(np.arange(len(patterns)), page_counts)

            def host_page():
                p = r.entries_by_id_packed(page_ids)
                data, o = p.data.tobytes(), p.offsets.tolist()
                return np.array([span(data[o[i]:o[i + 1]], patterns[int(pat_of[i])], 1, edits, icase) for i in range(page_ids.size)],
                                dtype=np.int32).reshape(-1, 3)

            device = {f'{tag}/near': lambda: r.search_near_ids_batch(patterns, 1, edits=edits, icase=icase).ids,
                      f'{tag}/spans_page': lambda: r.match_spans_batch(page_ids, page_counts, patterns, 1, edits, icase=icase),
                      f'{tag}/spans_all': lambda: r.match_spans_batch(all_ids, all_counts, patterns, 1, edits, icase=icase)}
            host = {f'{tag}/host_page': host_page}
            got, want = device[f'{tag}/spans_page'](), host_page()
            if not np.array_equal(got, want):
                bad = int(np.flatnonzero((got != want).any(axis=1))[0])
                raise SystemExit(f'{tag}: row {bad} is {got[bad].tolist()} on the device and {want[bad].tolist()} on the host')
            whole = device[f'{tag}/spans_all']()
            if not (whole[:, 2] >= 0).all() or not np.array_equal(whole[:page_ids.size][pat_of == 0], got[pat_of == 0]):
                raise SystemExit(f'{tag}: an id of the answer without a span, or the page differs from the whole')
            record = lambda out, st: {'rows': int(len(out))}
            mine = time_legs(device, lambda name: None, ap_args.warmup, ap_args.reps, ap_args.rounds, record=record)
            mine += time_legs(host, lambda name: None, 1, host_reps, ap_args.rounds, record=record)
            runs += mine
            summary.update(medians(mine, {**device, **host}))
            answers[tag] = {'ids': int(all_ids.size), 'page_rows': int(page_ids.size),
                            'page_distances': np.bincount(got[:, 2], minlength=2).tolist(),
                            'page_lengths_other_than_the_patterns': int((got[:, 1] != np.array([len(patterns[int(q)]) for q in pat_of])).sum())}
    r.close()
    med = {name: round(statistics.median(v), 4) for name, v in summary.items()}
    out = {'what': 'match_spans_batch on a page (the first ids of the near answer, with their patterns) and on the whole answer, vs '
                   'search_near_ids_batch alone (the call whose answer is explained), vs the route before: entries_by_id_packed of the page + '
                   'the per-row scoring of tests/span_ref.py in Python; k = 1, the four combinations of edits x icase; same reader: one 64 '
                   'MiB chunk of `words`; host clock around the whole leg, median / min / max over reps after warm-up; the legs alternate; '
                   'host_page was compared with spans_page row by row before the timing.  Not measured: k = 3, long entries, several chunks',
           'commit': ap_args.commit or commit_hash(), 'chunk_bytes': int(text.size), 'patterns': [p.decode() for p in patterns], 'k': 1,
           'page': ap_args.page, 'warmup': ap_args.warmup, 'reps': ap_args.reps, 'host_reps': host_reps, 'answers': answers, 'runs': runs,
           'summary': summary, 'median_of_medians_ms': med,
           'host_page_over_spans_page': {tag: round(med[f'{tag}/host_page'] / med[f'{tag}/spans_page'], 1) for tag in answers},
           'spans_all_over_near': {tag: round(med[f'{tag}/spans_all'] / med[f'{tag}/near'], 3) for tag in answers}}
    write_json(out, ap_args.out)
    print(json.dumps({'median_of_medians_ms': med, 'answers': answers, 'host_page_over_spans_page': out['host_page_over_spans_page'],
                      'spans_all_over_near': out['spans_all_over_near']}))


if __name__ == '__main__':
    main()
