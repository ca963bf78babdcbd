"""The arithmetic of the BFV monomial multiply and of the query expansion's odd children on the CPU (tests/csim/sim_bfv_expand.cpp runs
csrc/bfv_expand_core.h -- the source index and sign of a shift and (2c - even) mod q, the functions the HIP kernel k_bfv_shift compiles),
in both builds of the u64 engine, against Python integers:

* the shift map for every exponent e in [0, 2N) at N = 8 and N = 2048: coefficient i of the operand lands at (i + e) mod N, negated when
  (i + e) div N is odd (X^N = -1) -- the scatter the map's gather must invert;
* in * X^e at N = 8 against a schoolbook product mod (X^N + 1, q), operands with zeros: the negative of 0 is 0;
* (2c - even) mod q at c, even in {0, 1, q - 1, floor(q / 2)} for the chain primes of 40, 50 and 60 bits;
* the library without a device: the three entry points exist and are declared, he355_bfv_expand_galois_elts gives N / 2^j + 1, and a CKKS
  context, an exponent >= 2N, a bad size, a bad level and a bad count are refused with HE355_E_INVALID_ARGS on the host, before any device
  is asked for (valid arguments then fail with HE355_E_DEVICE and touch nothing).
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfvexp_shift_map.argtypes = [C.c_uint32, C.c_int, u32p, u32p]
    L.sim_bfvexp_shift_map.restype = None
    L.sim_bfvexp_shift.argtypes = [u64p, C.c_uint32, C.c_int, C.c_uint64, u64p]
    L.sim_bfvexp_shift.restype = None
    L.sim_bfvexp_odd.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.sim_bfvexp_odd.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


@pytest.mark.parametrize("logN", [3, 11])
def test_shift_map_for_every_exponent(sim, logN):
    N = 1 << logN
    i = np.arange(N)
    idx, neg = np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint32)
    for e in range(2 * N):
        sim.sim_bfvexp_shift_map(e, logN, idx.ctypes.data_as(u32p), neg.ctypes.data_as(u32p))
        # the scatter: operand coefficient i goes to (i + e) mod N with sign (-1)^((i + e) div N)
        want_idx, want_neg = np.empty(N, dtype=np.uint32), np.empty(N, dtype=np.uint32)
        want_idx[(i + e) % N] = i
        want_neg[(i + e) % N] = ((i + e) // N) & 1
        assert np.array_equal(idx, want_idx) and np.array_equal(neg, want_neg), e


def test_shift_equals_schoolbook_product(sim, be):
    N, logN = 8, 3
    ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=[60, 40, 60], plain_bits=20, sec128=False)
    rng = np.random.default_rng(8)
    for q in ctx.moduli:
        for kind in range(3):
            a = rng.integers(0, q, N, dtype=np.uint64)
            if kind == 1:
                a[::2] = 0
            if kind == 2:
                a[:] = [0, 1, q - 1, q // 2, 0, q - 1, 1, 0]
            for e in range(2 * N):
                want = [0] * N
                for i in range(N):  # a_i X^i * X^e, X^N = -1
                    k, sign = (i + e) % N, -1 if ((i + e) // N) & 1 else 1
                    want[k] = (want[k] + sign * int(a[i])) % q
                got = np.empty(N, dtype=np.uint64)
                sim.sim_bfvexp_shift(a.ctypes.data_as(u64p), e, logN, q, got.ctypes.data_as(u64p))
                assert got.tolist() == want, (q, kind, e)
    ctx.close()


def test_two_c_minus_even(sim, be):
    primes = set()
    for bits in ([60, 40, 60], [50, 40, 50]):
        ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=bits, plain_bits=20, sec128=False)
        primes |= set(ctx.moduli)
        ctx.close()
    assert {q.bit_length() for q in primes} == {40, 50, 60}
    for q in sorted(primes):
        edge = [0, 1, q - 1, q // 2]
        for c in edge:
            for even in edge:
                assert sim.sim_bfvexp_odd(c, even, q) == (2 * c - even) % q, (q, c, even)


# ---- the library without a device ----------------------------------------------------------------------------------------------
NEW = ["he355_bfv_multiply_monomial", "he355_bfv_expand_galois_elts", "he355_bfv_expand"]


def test_symbols_exported_and_declared(be):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])


def test_expand_galois_elts(be):
    N = 4096
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    assert ctx.bfv_expand_galois_elts(1) == []
    assert ctx.bfv_expand_galois_elts(2) == [N + 1]
    assert ctx.bfv_expand_galois_elts(5) == [N + 1, N // 2 + 1, N // 4 + 1]
    assert ctx.bfv_expand_galois_elts(8) == [N + 1, N // 2 + 1, N // 4 + 1]
    assert ctx.bfv_expand_galois_elts(N) == [N // (1 << j) + 1 for j in range(12)] and ctx.bfv_expand_galois_elts(N)[-1] == 3
    assert ctx.bfv_expand_galois_elts(0) == [] and ctx.bfv_expand_galois_elts(N + 1) == []
    buf = (C.c_uint32 * 2)(7, 7)  # cap: no more than cap entries are written, the count is still returned
    assert be.lib().he355_bfv_expand_galois_elts(ctx.h, 16, buf, 1) == 4 and list(buf) == [N + 1, 7]
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    assert ck.bfv_expand_galois_elts(8) == []
    ck.close()


def test_refusals_are_decided_on_the_host(be):
    N = 4096
    L = be.lib()
    buf = np.full(3 * 3 * N, 0xABCD, dtype=np.uint64)
    other = np.full(8 * 2 * 3 * N, 0xABCD, dtype=np.uint64)
    p, o = buf.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p)
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    Lt = ctx.L
    bad = [lambda: L.he355_bfv_multiply_monomial(ctx.h, Lt, 2, 1, p, 2 * N, o),
           lambda: L.he355_bfv_multiply_monomial(ctx.h, Lt, 0, 1, p, 1, o),
           lambda: L.he355_bfv_multiply_monomial(ctx.h, Lt, 4, 1, p, 1, o),
           lambda: L.he355_bfv_multiply_monomial(ctx.h, 0, 2, 1, p, 1, o),
           lambda: L.he355_bfv_multiply_monomial(ctx.h, Lt + 1, 2, 1, p, 1, o),
           lambda: L.he355_bfv_expand(ctx.h, Lt, 1, p, 0, o),
           lambda: L.he355_bfv_expand(ctx.h, Lt, 1, p, N + 1, o),
           lambda: L.he355_bfv_expand(ctx.h, 0, 1, p, 4, o),
           lambda: L.he355_bfv_expand(ctx.h, Lt + 1, 1, p, 4, o)]
    for k, f in enumerate(bad):
        assert f() == be.E_INVALID_ARGS, k
        assert len(L.he355_last_error()) > 0
    # valid arguments: there is no device behind this context, and no CPU fallback
    assert L.he355_bfv_multiply_monomial(ctx.h, Lt, 2, 1, p, 2 * N - 1, o) == be.E_DEVICE
    assert b"no CPU fallback" in L.he355_last_error()
    assert L.he355_bfv_expand(ctx.h, Lt, 1, p, 8, o) == be.E_DEVICE
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    assert L.he355_bfv_multiply_monomial(ck.h, ck.L, 2, 1, p, 1, o) == be.E_INVALID_ARGS
    assert b"BFV context" in L.he355_last_error()
    assert L.he355_bfv_expand(ck.h, ck.L, 1, p, 8, o) == be.E_INVALID_ARGS
    assert b"BFV context" in L.he355_last_error()
    ck.close()
    assert (buf == 0xABCD).all() and (other == 0xABCD).all()
