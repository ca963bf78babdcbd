"""The arithmetic of the scalar combination and the scalar-residue rule on the CPU (tests/csim/sim_poly.cpp runs csrc/poly_core.h -- the
functions the HIP kernel k_scalar_combine compiles, and he355_ckks_scalar_residues' rule) against Python integers, in both builds of the u64
engine:

* 1, 2, 255, 256, 257 and 513 terms under two 60-bit primes with every operand and every scalar q - 1 -- the 2^128 edge of a run: the
  constant opens the first run, so 255 products fill it -- and uniform ones; at the prime's own run length and at forced short ones;
* 14- to 31-bit primes; constants 0 and q - 1;
* the launch's run length is the shortest of its primes';
* scalar residues at +-0.5, +-1.5, +-2.5, 2^52 +- 1, 2^53 + 2, -2^90, 2^125, multiples of q, against int(round(v)) % q; non-finite
  scalars and magnitudes from 2^126 on are refused.
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import csim_lib

u64p = C.POINTER(C.c_uint64)
Q60 = [0xfffffffffff2801, 0xffffffffffc0001]
SMALL = [12289, 65537, 786433, 8380417, 1073479681, 2147352577]  # 14 to 31 bits
TERMS = [1, 2, 255, 256, 257, 513]


def declare(L):
    L.sim_poly_run.argtypes = [u64p, C.c_int]
    L.sim_poly_run.restype = C.c_uint64
    L.sim_poly_combine.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p]
    L.sim_poly_combine.restype = None
    L.sim_poly_scalar.argtypes = [C.c_double, u64p, C.c_int, u64p]
    L.sim_poly_scalar.restype = C.c_int
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def p64(a):
    return a.ctypes.data_as(u64p)


def check(sim, q, x, a, cst, runs):
    terms, n = x.shape
    want = [(sum(int(x[k, e]) * int(a[k]) for k in range(terms)) + cst) % q for e in range(n)]
    for run in runs:
        out = np.empty(n, dtype=np.uint64)
        sim.sim_poly_combine(n, q, terms, run, p64(np.ascontiguousarray(x)), p64(a), cst, p64(out))
        assert [int(v) for v in out] == want, (hex(q), terms, run, cst)


@pytest.mark.parametrize("q", Q60, ids=hex)
@pytest.mark.parametrize("terms", TERMS)
def test_the_combination_at_the_edge_of_a_run(sim, q, terms):
    assert (2 ** 128 - 1) // (q - 1) ** 2 == 256
    rng = np.random.default_rng(terms)
    n = 4
    full_x, full_a = np.full((terms, n), q - 1, dtype=np.uint64), np.full(terms, q - 1, dtype=np.uint64)
    uni_x, uni_a = rng.integers(0, q, (terms, n), dtype=np.uint64), rng.integers(0, q, terms, dtype=np.uint64)
    for x, a in ((full_x, full_a), (uni_x, uni_a), (full_x, uni_a)):
        for cst in (0, q - 1):
            check(sim, q, x, a, cst, (0, 2, 3, 256))


@pytest.mark.parametrize("q", SMALL)
def test_the_combination_under_small_primes(sim, q):
    rng = np.random.default_rng(q)
    for terms in (1, 2, 257):
        x, a = rng.integers(0, q, (terms, 4), dtype=np.uint64), rng.integers(0, q, terms, dtype=np.uint64)
        for cst in (0, q - 1):
            check(sim, q, x, a, cst, (0, 2))
            check(sim, q, np.full((terms, 4), q - 1, dtype=np.uint64), np.full(terms, q - 1, dtype=np.uint64), cst, (0, 5))


def test_the_run_length_of_a_launch(sim):
    for chain, run in ((Q60 + [SMALL[5]], 256), (SMALL, 1 << 16), ([SMALL[0], Q60[1]], 256)):
        qs = np.array(chain, dtype=np.uint64)
        assert sim.sim_poly_run(p64(qs), len(chain)) == run


def test_scalar_residues_against_python_round(sim):
    qs = np.array(Q60 + SMALL + [0xffffff7801], dtype=np.uint64)
    q0 = int(qs[0])
    values = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, 1e-300, 3.0, -7.0, 2.0 ** 52 - 1, 2.0 ** 52 + 1, -(2.0 ** 52 + 1), 2.0 ** 52 - 0.5,
              2.0 ** 53 + 2, -(2.0 ** 90), 2.0 ** 125, -(2.0 ** 125), math.nextafter(2.0 ** 126, 0.0), float(q0), float(-q0), 3.0 * SMALL[0], -5.0 * SMALL[3],
              2.0 ** 60 * 3.7, 1234567.5, 1234568.5, -1e30]
    out = np.empty(len(qs), dtype=np.uint64)
    for v in values:
        assert sim.sim_poly_scalar(v, p64(qs), len(qs), p64(out)) == 1, v
        assert [int(x) for x in out] == [int(round(v)) % int(q) for q in qs], v
    for v in (float("inf"), float("-inf"), float("nan"), 2.0 ** 126, -(2.0 ** 126), 1e300):
        assert sim.sim_poly_scalar(v, p64(qs), len(qs), p64(out)) == 0, v
