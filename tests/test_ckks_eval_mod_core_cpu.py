"""The per-lane arithmetic of the fused combine-and-rescale step on the CPU (tests/csim/sim_cheb.cpp runs csrc/cheb_core.h -- the functions
the HIP kernels k_scalar_combine_row and k_floor_rows_combine compile) against Python integers, in both builds of the u64 engine and in
the fp64 engine:

* the lane sums at 1, 2, 255, 256, 257 and 513 terms under two 60-bit primes with every operand and every scalar q - 1 -- the 2^128 edge of
  a run -- and uniform ones, constants 0 and q - 1, at the prime's own run length and at forced short ones; small primes;
* the fused element  ((sum_t a_t x_t + c) - corr) * q_s^-1 mod q_i  in the u64 engine (corr a lazy value: 0, q - 1, 4q - 1, uniform below 4q)
  under 60-bit targets in both builds and under narrower ones in the Shoup build, and in the fp64 engine (corr a centred double with
  |corr| <= q - 1) under primes of 30 to 46 bits -- with q - 1 operands, q - 1 scalars and a 257-term run.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import csim_lib
import oracle as ho

u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
Q60 = [0xfffffffffff2801, 0xffffffffffc0001]
SMALL = [12289, 786433, 1073479681, 2147352577]
F64Q = [1073479681, 0xffffff7801] + sorted(ho.Context(ho.SCHEME_CKKS, 2048, bit_sizes=[42, 38, 45, 46], sec128=False).moduli[2:])  # 30, 40, 45, 46 bits
TERMS = [1, 2, 255, 256, 257, 513]


def declare(L):
    sums = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p]
    L.sim_cheb_sums.argtypes = sums
    L.sim_cheb_sums.restype = None
    L.sim_cheb_fused_u64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p, u64p]
    L.sim_cheb_fused_u64.restype = None
    L.sim_cheb_fused_f64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, f64p, u64p]
    L.sim_cheb_fused_f64.restype = None
    L.sim_cheb_form.restype = C.c_int
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = declare(csim_lib.load(fold=request.param))
    assert L.sim_cheb_form() == int(request.param)
    return L


def p64(a):
    return a.ctypes.data_as(u64p)


def sums(x, a, cst, q):
    terms, n = x.shape
    return [(sum(int(x[k, e]) * int(a[k]) for k in range(terms)) + cst) % q for e in range(n)]


def operand_sets(rng, q, terms, n):
    full_x, full_a = np.full((terms, n), q - 1, dtype=np.uint64), np.full(terms, q - 1, dtype=np.uint64)
    uni_x, uni_a = rng.integers(0, q, (terms, n), dtype=np.uint64), rng.integers(0, q, terms, dtype=np.uint64)
    return (full_x, full_a), (uni_x, uni_a), (full_x, uni_a)


@pytest.mark.parametrize("q", Q60 + SMALL, ids=hex)
@pytest.mark.parametrize("terms", TERMS)
def test_the_lane_sums_at_the_edge_of_a_run(sim, q, terms):
    rng = np.random.default_rng(terms)
    n = 8
    for x, a in operand_sets(rng, q, terms, n):
        for cst in (0, q - 1):
            want = sums(x, a, cst, q)
            for run in (0, 2, 3, 256):
                out = np.empty(n, dtype=np.uint64)
                sim.sim_cheb_sums(n, q, terms, run, p64(np.ascontiguousarray(x)), p64(a), cst, p64(out))
                assert [int(v) for v in out] == want, (hex(q), terms, run, cst)


def fused_want(x, a, cst, corr, qi, qs):
    inv = pow(qs % qi, -1, qi)
    return [((s - int(c)) * inv) % qi for s, c in zip(sums(x, a, cst, qi), corr)]


@pytest.mark.parametrize("terms", [1, 2, 257])
def test_the_fused_element_in_the_u64_engine(sim, terms):
    fold = sim.sim_cheb_form() == 1
    targets = Q60 if fold else Q60 + SMALL + F64Q[1:]
    n = 8
    for qi in targets:
        rng = np.random.default_rng(qi % 1000 + terms)
        for qs in (Q60[1] if qi == Q60[0] else Q60[0], 0xffffff7801 if qi != 0xffffff7801 else 1073479681):
            for x, a in operand_sets(rng, qi, terms, n):
                for cst in (0, qi - 1):
                    corr = np.array([0, qi - 1, 4 * qi - 1, qi, 2 * qi] + [int(v) for v in rng.integers(0, 4 * qi, n - 5, dtype=np.uint64)], dtype=np.uint64)
                    out = np.empty(n, dtype=np.uint64)
                    sim.sim_cheb_fused_u64(n, qi, qs, terms, 0, p64(np.ascontiguousarray(x)), p64(a), cst, p64(corr), p64(out))
                    assert [int(v) for v in out] == fused_want(x, a, cst, corr, qi, qs), (hex(qi), hex(qs), terms, cst)


@pytest.mark.parametrize("terms", [1, 2, 257])
def test_the_fused_element_in_the_fp64_engine(sim, terms):
    n = 8
    for qi in F64Q:
        rng = np.random.default_rng(qi % 1000 + terms)
        for qs in (Q60[0], F64Q[0] if qi != F64Q[0] else F64Q[1]):
            for x, a in operand_sets(rng, qi, terms, n):
                for cst in (0, qi - 1):
                    ints = [0, qi - 1, -(qi - 1), 1, -1] + [int(v) - (qi - 1) for v in rng.integers(0, 2 * qi - 1, n - 5, dtype=np.uint64)]
                    corr = np.array([float(v) for v in ints], dtype=np.float64)
                    out = np.empty(n, dtype=np.uint64)
                    sim.sim_cheb_fused_f64(n, qi, qs, terms, 0, p64(np.ascontiguousarray(x)), p64(a), cst, corr.ctypes.data_as(f64p), p64(out))
                    assert [int(v) for v in out] == fused_want(x, a, cst, ints, qi, qs), (hex(qi), hex(qs), terms, cst)
