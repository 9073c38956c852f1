"""Helpers shared by the parity tests: call the C ABI on host buffers."""
import ctypes

import numpy as np

from pysubstringsearch_amd import _ffi


def sa_gpu(data, device: int = 0) -> np.ndarray:
    """pss_sa_build (host pointers in, host pointers out) -> int32 array."""
    t = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if not isinstance(data, np.ndarray) else \
        np.ascontiguousarray(data, dtype=np.uint8)
    sa = np.full(t.size, -1, dtype=np.int32)
    buf = t if t.size else np.zeros(1, np.uint8)
    out = sa if sa.size else np.zeros(1, np.int32)
    rc = _ffi.lib.pss_sa_build(buf.ctypes.data, out.ctypes.data, t.size, device)
    _ffi.check(rc)
    return sa


def gen_corpus(kind: int, n: int, chunk_index: int = 0) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    _ffi.check(_ffi.lib.pss_gen_corpus(kind, out.ctypes.data, n, chunk_index))
    return out


def sa_device(host, stats=None, flags=0):
    """Suffix array of a text built where it lies, in HBM (pss_sa_build_device); `stats` takes the build's SaStats."""
    import torch
    n = host.size
    dT = torch.from_numpy(host).cuda()
    dSA = torch.empty(n, dtype=torch.int32, device='cuda')
    st = _ffi.SaStats()
    _ffi.check(_ffi.lib.pss_sa_build_device(dT.data_ptr(), dSA.data_ptr(), n, 0, flags, ctypes.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return dSA.cpu().numpy()


def kat_input(k):
    """The text of one known-answer test of tests/golden/sa_kats.json, by its name."""
    fib = [b'a', b'ab']
    while len(fib[-1]) < 987:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(12345)
    perm = rng.permutation(256).astype(np.uint8).tobytes()
    zfn = np.array([0, 255, 10], dtype=np.uint8)[rng.integers(0, 3, 4096)].tobytes()
    table = {
        'a1000_nl': b'a' * 1000 + b'\n', 'fibonacci_987': fib[-1], 'perm256': perm, 'zero_ff_nl_4k': zfn,
        'periodic_64x64': (b'a' * 63 + b'\n') * 64, 'all_zero_5000': b'\x00' * 5000,
        'zeros_tail': b'\xff' * 4097 + b'\x00' * 17,
        'readme_chunk': b'some short string\nanother but now a longer string\nmore text to add\n',
    }
    if k['name'] in table:
        return table[k['name']]
    kinds = {'lines_1MiB': 0, 'words_1MiB': 1, 'runs_1MiB': 2, 'periodic_1MiB': 3}
    return gen_corpus(kinds[k['name']], 1 << 20).tobytes()
