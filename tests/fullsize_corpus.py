"""The corpora of tests/test_fullsize_gpu.py: generated chunks, their suffix arrays built on the GPU and checked against
the goldens of tests/golden/sa_big.json, a reader that holds them, and the query batch of the benchmark over them.  Also
what tests/tools/words_counts.py measures on."""
import ctypes

import numpy as np

import bench
from pysubstringsearch_amd import Reader, _ffi

GOLD = bench.load_big_goldens()
def _build_device(host: np.ndarray):
    import torch
    n = host.size
    dT = torch.from_numpy(host).cuda()
    dSA = torch.empty(n, dtype=torch.int32, device='cuda')
    st = _ffi.SaStats()
    _ffi.check(_ffi.lib.pss_sa_build_device(dT.data_ptr(), dSA.data_ptr(), n, 0, 0, ctypes.byref(st)))
    return dT, dSA, st.as_dict()


def _gen(kind: str, n: int, chunk: int = 0) -> np.ndarray:
    host = np.empty(n, dtype=np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus(bench.KINDS[kind], host.ctypes.data, n, chunk))
    return host


def _corpus_reader(logn: int, chunks: int, keep_sa: bool, oracle=None, check_libsais_live: bool = False, kind: str = 'lines'):
    """`chunks` chunks of the `kind` corpus built on the GPU and made resident through the device hand-off."""
    n = 1 << logn
    h = ctypes.c_void_p()
    _ffi.check(_ffi.lib.pss_reader_create(0, ctypes.byref(h)))
    reader = Reader._from_handle(h)
    texts, sas = [], []
    for c in range(chunks):
        host = _gen(kind, n, c)
        dT, dSA, _ = _build_device(host)
        g = GOLD.get((kind, c, n))
        if g is not None:
            assert bench.sa_poly64_torch(dSA) == g['sa_poly64'], f'chunk {c}: suffix array differs from libsais'
        _ffi.check(_ffi.lib.pss_reader_add_chunk_device(h, dT.data_ptr(), dSA.data_ptr(), n))
        texts.append(host)
        if keep_sa:
            sa = dSA.cpu().numpy()
            if check_libsais_live:
                assert np.array_equal(sa, oracle.sa(host)), f'chunk {c}'
            sas.append(sa)
        del dT, dSA
    return reader, texts, sas


def _batch(texts, nq, qmin=4):
    chunks = len(texts)
    per = (nq // 2 + chunks - 1) // chunks
    sampled = [q for c, t in enumerate(texts) for q in bench.sample_chunk_queries(t, c, per, qmin, 32)]
    return bench.mixed_queries(sampled, nq, qmin, 32)
