"""The arithmetic of the baby-step/giant-step linear transform on the CPU (tests/csim/sim_bsgs.cpp runs csrc/bsgs_core.h -- the functions
the HIP kernels k_hoist_rot_qp, k_bsgs_ident and k_bsgs_inner compile) against Python integers, in both builds of the u64 engine:

* the folded term s + P c0, the identity baby's P c and the giant accumulate, at uniform operands, 0 and q - 1, under a 60-, a 50- and a
  40-bit prime with a 60- and a 50-bit special prime;
* the inner sum at 1, 255, 256, 257 and 511 terms of all q - 1 (and uniform ones) under a 60-bit, a 50-bit and a 40-bit prime: both sides of
  every run boundary of the 60-bit prime (256 terms, then 255 new ones per run), at the prime's own run length and at forced short ones --
  the result does not depend on where the runs are cut;
* the run rule itself: no fold up to `run` terms, then one per run - 1 new terms; the launch's run length is the shortest of its primes'.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import csim_lib

u64p = C.POINTER(C.c_uint64)
PRIMES = {60: 0xfffffffffff2801, 50: 0x3ffffffffa801, 40: 0xffffff7801}
SPECIAL = [0xffffffffffc0001, 0x3ffffffff0001]
TERMS = [1, 255, 256, 257, 511]


def declare(L):
    L.sim_bsgs_p_mod.argtypes = [C.c_uint64, C.c_uint64]
    L.sim_bsgs_p_mod.restype = C.c_uint64
    L.sim_bsgs_fold_c0.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, u64p]
    L.sim_bsgs_fold_c0.restype = None
    L.sim_bsgs_ident.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
    L.sim_bsgs_ident.restype = None
    L.sim_bsgs_acc.argtypes = [C.c_uint64, C.c_uint64, u64p, u64p, u64p]
    L.sim_bsgs_acc.restype = None
    L.sim_bsgs_run.argtypes = [u64p, C.c_int]
    L.sim_bsgs_run.restype = C.c_uint64
    L.sim_bsgs_inner.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, u64p]
    L.sim_bsgs_inner.restype = None
    L.sim_bsgs_folds.argtypes = [C.c_uint64, C.c_uint64]
    L.sim_bsgs_folds.restype = C.c_uint64
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def p64(a):
    return a.ctypes.data_as(u64p)


def ints(a):
    return [int(x) for x in a]


@pytest.mark.parametrize("bits", list(PRIMES))
def test_the_folded_c0_term_against_python_integers(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(400 + bits)
    n = 64
    for P in SPECIAL:
        assert sim.sim_bsgs_p_mod(P, q) == P % q
        uni = lambda: rng.integers(0, q, n, dtype=np.uint64)
        full, zero = np.full(n, q - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for s, c in ((uni(), uni()), (full, full), (zero, full), (full, zero), (zero, zero)):
            out = np.empty(n, dtype=np.uint64)
            sim.sim_bsgs_fold_c0(n, q, P, p64(s), p64(c), p64(out))
            assert ints(out) == [(a + P * b) % q for a, b in zip(ints(s), ints(c))]
            sim.sim_bsgs_ident(n, q, P, p64(c), p64(out))
            assert ints(out) == [(P * b) % q for b in ints(c)]
            sim.sim_bsgs_acc(n, q, p64(s), p64(c), p64(out))
            assert ints(out) == [(a + b) % q for a, b in zip(ints(s), ints(c))]


@pytest.mark.parametrize("bits", list(PRIMES))
@pytest.mark.parametrize("terms", TERMS)
def test_the_inner_sum_on_both_sides_of_every_run_boundary(sim, bits, terms):
    q = PRIMES[bits]
    rng = np.random.default_rng(bits * 1000 + terms)
    n = 8
    full = np.full((terms, n), q - 1, dtype=np.uint64)
    uni_t, uni_p = rng.integers(0, q, (terms, n), dtype=np.uint64), rng.integers(0, q, (terms, n), dtype=np.uint64)
    for t, p in ((full, full), (uni_t, uni_p), (full, uni_p)):
        want = [sum(int(t[k, e]) * int(p[k, e]) for k in range(terms)) % q for e in range(n)]
        for run in (0, 2, 3, 256 if bits == 60 else 255):  # the prime's own run, and short ones (every prime takes at least 256 terms)
            out = np.empty(n, dtype=np.uint64)
            sim.sim_bsgs_inner(n, q, terms, run, p64(np.ascontiguousarray(t)), p64(np.ascontiguousarray(p)), p64(out))
            assert ints(out) == want, (bits, terms, run)


def test_the_run_rule(sim):
    q60 = PRIMES[60]
    assert (2 ** 128 - 1) // (q60 - 1) ** 2 == 256  # the 60-bit prime's run
    for terms, folds in ((1, 0), (255, 0), (256, 0), (257, 1), (511, 1), (512, 2), (766, 2), (767, 3)):
        assert sim.sim_bsgs_folds(terms, 256) == folds, terms
    assert sim.sim_bsgs_folds(5, 2) == 3  # a run of two: the carried residue and one new term
    for chain, run in (([60, 40, 50], 256), ([50, 40], 1 << 16), ([40, 60], 256)):
        qs = np.array([PRIMES[b] for b in chain], dtype=np.uint64)
        assert sim.sim_bsgs_run(p64(qs), len(chain)) == run, chain
