"""The arithmetic of a level of the BFV ciphertext merge on the CPU (tests/csim/sim_bfv_merge.cpp runs csrc/bfv_merge_core.h over the shift
map of csrc/bfv_expand_core.h -- the functions the HIP kernel k_bfv_merge compiles), in both builds of the u64 engine, against Python
integers:

* S = even + X^s odd and D = even - X^s odd mod (X^N + 1, q) for every s = 2^j, j < log2 N (s = 1, the kernel's ODD form, and s = N / 2
  included), at N = 1024 and N = 2048, for chain primes of 40, 50 and 60 bits; operands all 0, all q - 1 and uniform, in every pairing, so
  that -0 = 0, the wrap of the sum and the borrow of the difference occur under both signs of the shift;
* one coefficient at even, odd in {0, 1, q - 1, floor(q / 2)} under both signs;
* the library without a device: the entry point exists, is declared and bound.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfvmerge_level.argtypes = [u64p, u64p, C.c_uint32, C.c_int, C.c_uint64, u64p, u64p]
    L.sim_bfvmerge_level.restype = None
    L.sim_bfvmerge_pair.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, u64p]
    L.sim_bfvmerge_pair.restype = None
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


@pytest.fixture(scope="module")
def primes(be):
    out = set()
    for bits in ([60, 40, 60], [50, 40, 50]):
        ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=bits, plain_bits=20, sec128=False)
        out |= set(ctx.moduli)
        ctx.close()
    assert {q.bit_length() for q in out} == {40, 50, 60}
    return sorted(out)


def want_level(even, odd, s, q):
    """Python integers: coefficient i of odd goes to i + s, negated past X^N"""
    N = len(even)
    e, o = even.astype(object), odd.astype(object)
    m = np.empty(N, dtype=object)
    m[s:] = o[:N - s]
    m[:s] = -o[N - s:]
    return ((e + m) % q).astype(np.uint64), ((e - m) % q).astype(np.uint64)


@pytest.mark.parametrize("logN", [10, 11])
def test_level_for_every_shift(sim, primes, logN):
    N = 1 << logN
    rng = np.random.default_rng(9 + logN)
    for q in primes:
        kinds = {"zero": np.zeros(N, dtype=np.uint64), "top": np.full(N, q - 1, dtype=np.uint64), "uniform": rng.integers(0, q, N, dtype=np.uint64)}
        for j in range(logN):
            s = 1 << j
            for ke, even in kinds.items():
                for ko, odd in kinds.items():
                    S, D = np.empty(N, dtype=np.uint64), np.empty(N, dtype=np.uint64)
                    sim.sim_bfvmerge_level(even.ctypes.data_as(u64p), odd.ctypes.data_as(u64p), s, logN, q, S.ctypes.data_as(u64p), D.ctypes.data_as(u64p))
                    wS, wD = want_level(even, odd, s, q)
                    assert np.array_equal(S, wS) and np.array_equal(D, wD), (q, s, ke, ko)


def test_pair_at_the_edges(sim, primes):
    out = (C.c_uint64 * 2)()
    for q in primes:
        edge = [0, 1, q - 1, q // 2]
        for even in edge:
            for odd in edge:
                for neg in (0, 1):
                    sim.sim_bfvmerge_pair(even, odd, neg, q, out)
                    m = -odd if neg else odd
                    assert (out[0], out[1]) == ((even + m) % q, (even - m) % q), (q, even, odd, neg)


def test_symbol_exported_declared_and_bound(be):
    s = "he355_bfv_merge"
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    assert hasattr(lib, s)
    assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
    assert hasattr(be.Context, "bfv_merge")
