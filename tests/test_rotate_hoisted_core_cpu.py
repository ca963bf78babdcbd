"""The finish arithmetic of the hoisted rotations on the CPU (tests/csim/sim_hoist.cpp runs csrc/hoist_core.h -- the functions the HIP kernels
k_hoist_finish_ntt and k_hoist_finish_coeff compile -- over whole residue polynomials in the kernels' order: the ONE source row of a row, read
whole, joined, permuted) against Python integers, in both builds of the u64 engine, under a 60-, a 50-, a 40- and a 35-bit prime, at N = 1024
(one row), 2048 and 8192, for the elements 3, 3^-1, 9, 2N - 1 and 1:

* polynomial 0 is perm(c0 + u), polynomial 1 perm(u), the identity's term perm(c0) alone -- with uniform operands, all q - 1 (every sum wraps),
  all 0, and u = q - c0 (every sum is exactly q, which reduces to 0); the permutation itself is the oracle's apply_galois_poly in NTT form;
* the plain sum's term acc + plain * v at uniform operands and at all q - 1 (the largest product and a sum that wraps), first and later terms;
* the signed gather is the oracle's apply_galois_poly in coefficient form, zeros included (-0 = 0, not q).
No GPU."""
import ctypes as C

import numpy as np
import pytest

import csim_lib

u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
PRIMES = {60: 0xfffffffffff2801, 50: 0x3ffffffffa801, 40: 0xffffff7801, 35: 0x7ffffc801}
RINGS = (1024, 2048, 8192)


def declare(L):
    L.sim_hoist_table.argtypes = [C.c_uint64, C.c_uint32, C.c_int, u32p]
    L.sim_hoist_table.restype = None
    L.sim_hoist_finish_ntt.argtypes = [C.c_uint64, C.c_uint64, u32p, u64p, u64p, C.c_int, u64p, C.c_int, u64p]
    L.sim_hoist_finish_ntt.restype = None
    L.sim_hoist_finish_coeff.argtypes = [C.c_uint64, C.c_uint64, u32p, u64p, u64p]
    L.sim_hoist_finish_coeff.restype = None
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def p64(a):
    return a.ctypes.data_as(u64p) if a is not None else None


def table(sim, N, elt, mode):
    t = np.empty(N, dtype=np.uint32)
    sim.sim_hoist_table(N, elt, mode, t.ctypes.data_as(u32p))
    return t


def elements(N):
    return [3, pow(3, -1, 2 * N), 9, 2 * N - 1, 1]


def finish_ntt(sim, N, q, perm, u, c0, poly0, plain=None, first=True, out=None):
    out = np.zeros(N, dtype=np.uint64) if out is None else out.copy()
    sim.sim_hoist_finish_ntt(N, q, perm.ctypes.data_as(u32p), p64(u), p64(c0), int(poly0), p64(plain), int(first), p64(out))
    return out


def ints(a):
    return [int(x) for x in a]


@pytest.mark.parametrize("N", RINGS)
def test_the_permutation_is_the_oracles_and_every_row_has_one_source_row(sim, oracle, N):
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=[50, 60], sec128=False)
    x = np.arange(N, dtype=np.uint64) + np.uint64(7)
    for g in elements(N):
        perm = table(sim, N, g, 0)
        assert sorted(ints(perm)) == list(range(N)), g
        assert all(len(set(ints(perm[a:a + 1024] >> 10))) == 1 for a in range(0, N, 1024)), g
        assert np.array_equal(x[perm], o.apply_galois_poly(0, g, 1, x)), g
        got = finish_ntt(sim, N, PRIMES[50], perm, x, None, False)
        assert np.array_equal(got, x[perm]), g


@pytest.mark.parametrize("bits", list(PRIMES))
def test_join_and_permute_against_python_integers(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits)
    for N in RINGS:
        full, zero = np.full(N, q - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        c_r, u_r = rng.integers(0, q, N, dtype=np.uint64), rng.integers(0, q, N, dtype=np.uint64)
        u_neg = (np.uint64(q) - c_r) % np.uint64(q)
        for g in elements(N)[:4 if N > 1024 else 5]:
            perm = ints(table(sim, N, g, 0))
            pt = table(sim, N, g, 0)
            for u, c in ((u_r, c_r), (full, full), (zero, zero), (u_neg, c_r), (full, zero), (zero, full)):
                ui, ci = ints(u), ints(c)
                assert ints(finish_ntt(sim, N, q, pt, u, c, True)) == [(ui[s] + ci[s]) % q for s in perm], (N, g)
                assert ints(finish_ntt(sim, N, q, pt, u, c, False)) == [ui[s] for s in perm], (N, g)
                assert ints(finish_ntt(sim, N, q, pt, None, c, True)) == [ci[s] for s in perm], (N, g)


@pytest.mark.parametrize("bits", list(PRIMES))
def test_plain_term_against_python_integers(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(100 + bits)
    N = 2048
    g = 9
    pt = table(sim, N, g, 0)
    perm = ints(pt)
    full = np.full(N, q - 1, dtype=np.uint64)
    for u, c, pl, acc in ((rng.integers(0, q, N, dtype=np.uint64), rng.integers(0, q, N, dtype=np.uint64), rng.integers(0, q, N, dtype=np.uint64),
                           rng.integers(0, q, N, dtype=np.uint64)), (full, full, full, full), (full, np.zeros(N, dtype=np.uint64), full, full)):
        ui, ci, pi, ai = ints(u), ints(c), ints(pl), ints(acc)
        for poly0 in (True, False):
            v = [(ui[s] + (ci[s] if poly0 else 0)) % q for s in perm]
            assert ints(finish_ntt(sim, N, q, pt, u, c, poly0, pl, True, acc)) == [(v[e] * pi[e]) % q for e in range(N)]  # first: acc is not read
            assert ints(finish_ntt(sim, N, q, pt, u, c, poly0, pl, False, acc)) == [(ai[e] + v[e] * pi[e]) % q for e in range(N)]
        # the identity as a term: plain * c0's polynomial itself
        ident = table(sim, N, 1, 0)
        assert ints(finish_ntt(sim, N, q, ident, None, c, True, pl, False, acc)) == [(ai[e] + ci[e] * pi[e]) % q for e in range(N)]


@pytest.mark.parametrize("N", RINGS)
def test_signed_gather_is_the_oracles_coefficient_map(sim, oracle, N):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=[50, 60], plain_bits=20, sec128=False)
    q = o.moduli[0]
    rng = np.random.default_rng(N)
    x = rng.integers(0, q, N, dtype=np.uint64)
    x[::7] = 0
    x[1::7] = q - 1
    for g in elements(N):
        gt = table(sim, N, g, 1)
        out = np.empty(N, dtype=np.uint64)
        sim.sim_hoist_finish_coeff(N, q, gt.ctypes.data_as(u32p), p64(x), p64(out))
        assert np.array_equal(out, o.apply_galois_poly(0, g, 0, x)), g
        assert int(out.max()) < q
