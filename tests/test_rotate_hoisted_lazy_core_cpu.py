"""The arithmetic of the lazy plain sum and of the plaintext extension on the CPU (tests/csim/sim_hoist_lazy.cpp runs csrc/hoist_core.h -- the
functions the HIP kernels k_hoist_acc_qp and k_plain_extend compile -- over whole residue polynomials in the kernels' order) against Python
integers, in both builds of the u64 engine, under a 60-, a 50-, a 40- and a 35-bit prime (u64- and fp64-engine sizes):

* the tile's prime: the data primes, then the special prime;
* one term of an accumulator, acc + plain * sigma(v), keyed (the ONE source row of each row) and the identity's, first and later terms, at
  uniform operands, all 0 and all q - 1 (the largest product on the largest accumulator: the sum wraps); the order of the terms does not matter;
* the constant the forward row pass of an unnormalised inverse row pass leaves: fix * 1024 = 1 mod q, and times it at 0, q - 1 and uniform;
* the centred reduction of a coefficient at 0, floor(q_0 / 2) (the last positive one), floor(q_0 / 2) + 1 (the first negative one), q_0 - 1,
  multiples of the target prime and uniform values, into a smaller, an equal-sized and a larger prime.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import csim_lib

u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
PRIMES = {60: 0xfffffffffff2801, 50: 0x3ffffffffa801, 40: 0xffffff7801, 35: 0x7ffffc801}


def declare(L):
    L.sim_hoist_table.argtypes = [C.c_uint64, C.c_uint32, C.c_int, u32p]
    L.sim_hoist_table.restype = None
    L.sim_hoist_qp_prime.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sim_hoist_qp_prime.restype = C.c_int
    L.sim_hoist_acc_qp.argtypes = [C.c_uint64, C.c_uint64, u32p, u64p, u64p, C.c_int, u64p]
    L.sim_hoist_acc_qp.restype = None
    L.sim_hoist_row_pass_fix.argtypes = [C.c_uint64]
    L.sim_hoist_row_pass_fix.restype = C.c_uint64
    L.sim_hoist_sp_unscale.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
    L.sim_hoist_sp_unscale.restype = None
    L.sim_hoist_centred_mod.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
    L.sim_hoist_centred_mod.restype = None
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def p64(a):
    return a.ctypes.data_as(u64p)


def ints(a):
    return [int(x) for x in a]


def table(sim, N, elt):
    t = np.empty(N, dtype=np.uint32)
    sim.sim_hoist_table(N, elt, 0, t.ctypes.data_as(u32p))
    return t


def acc_qp(sim, N, q, perm, src, plain, first, acc):
    out = acc.copy()
    sim.sim_hoist_acc_qp(N, q, perm.ctypes.data_as(u32p) if perm is not None else None, p64(src), p64(plain), int(first), p64(out))
    return out


def test_the_tiles_prime(sim):
    for L, K in ((1, 2), (3, 4), (2, 4), (16, 17)):
        assert [sim.sim_hoist_qp_prime(i, L, K) for i in range(L + 1)] == list(range(L)) + [K - 1]


@pytest.mark.parametrize("bits", list(PRIMES))
def test_accumulator_terms_against_python_integers(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(200 + bits)
    for N in (1024, 2048, 8192):
        uni = lambda: rng.integers(0, q, N, dtype=np.uint64)
        full, zero = np.full(N, q - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
        for g in (3, pow(3, -1, 2 * N), 2 * N - 1):
            pt = table(sim, N, g)
            perm = ints(pt)
            for v, pl, acc in ((uni(), uni(), uni()), (full, full, full), (zero, full, full), (full, zero, zero), (uni(), full, zero)):
                vi, pi, ai = ints(v), ints(pl), ints(acc)
                assert ints(acc_qp(sim, N, q, pt, v, pl, True, acc)) == [(vi[perm[e]] * pi[e]) % q for e in range(N)], (N, g)  # first: acc is not read
                assert ints(acc_qp(sim, N, q, pt, v, pl, False, acc)) == [(ai[e] + vi[perm[e]] * pi[e]) % q for e in range(N)], (N, g)
                assert ints(acc_qp(sim, N, q, None, v, pl, False, acc)) == [(ai[e] + vi[e] * pi[e]) % q for e in range(N)], N  # the identity's term
    # the order of the terms does not matter: canonical in, canonical out
    N = 2048
    terms = [(table(sim, N, g), rng.integers(0, q, N, dtype=np.uint64), rng.integers(0, q, N, dtype=np.uint64)) for g in (3, 9, 27, 2 * N - 1)]
    sums = []
    for order in ((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0)):
        acc = np.zeros(N, dtype=np.uint64)
        for k, i in enumerate(order):
            acc = acc_qp(sim, N, q, terms[i][0], terms[i][1], terms[i][2], k == 0, acc)
        sums.append(acc)
    assert np.array_equal(sums[0], sums[1]) and np.array_equal(sums[0], sums[2])


@pytest.mark.parametrize("bits", list(PRIMES))
def test_the_row_pass_constant(sim, bits):
    q = PRIMES[bits]
    fix = sim.sim_hoist_row_pass_fix(q)
    assert 0 < fix < q and (fix * 1024) % q == 1
    rng = np.random.default_rng(300 + bits)
    v = rng.integers(0, q, 64, dtype=np.uint64)
    v[0], v[1], v[2] = 0, q - 1, 1024 % q
    out = np.empty_like(v)
    sim.sim_hoist_sp_unscale(len(v), q, fix, p64(v), p64(out))
    assert ints(out) == [(x * fix) % q for x in ints(v)]
    assert all((y * 1024) % q == x for x, y in zip(ints(v), ints(out)))


@pytest.mark.parametrize("bits0", list(PRIMES))
@pytest.mark.parametrize("bits", list(PRIMES))
def test_centred_reduction_against_python_integers(sim, bits0, bits):
    q0, q = PRIMES[bits0], PRIMES[bits]
    rng = np.random.default_rng(bits0 * 64 + bits)
    c = rng.integers(0, q0, 256, dtype=np.uint64)
    edge = [0, 1, q0 // 2 - 1, q0 // 2, q0 // 2 + 1, q0 - 1, q % q0, (q0 - q) % q0, (2 * q) % q0, (q0 - 2 * q) % q0]
    c[:len(edge)] = edge
    out = np.empty_like(c)
    sim.sim_hoist_centred_mod(len(c), q0, q, p64(c), p64(out))
    want = [(x if x <= q0 // 2 else x - q0) % q for x in ints(c)]
    assert ints(out) == want
    assert int(out.max()) < q
