"""The arithmetic of seeded BFV queries and Galois keys on the CPU (tests/csim/sim_bfv_seeded.cpp runs csrc/bfv_seeded_core.h -- the functions the
HIP kernels k_bfv_seeded_gen and k_bfv_seeded_finish compile) against Python integers, in both builds of the u64 engine:

* the uniform draw -- base word hoisted, limit made on the host, Barrett reduction in the place of `%` -- equals the accepted 64-bit draw of the
  restated sampler (tests/bfv_seeded_ref.py) reduced with Python's %, for every prime of every chain of bfv_gpu_helpers.ALL, the primes of
  {45, 55, 50} and a generic (not 2^60 - c) 60-bit prime: at the first 4096 coefficients, at a coefficient whose first draw is rejected under a
  BUILT seed (every prime), and at every coefficient of a search of 2^20 that takes a second draw on the generic prime, where rejection has
  probability 2^-4.9 >= 2^-14 -- the test asserts the search found some;
* the Barrett reduction alone at 0, 1, q - 1, q, q + 1, 2 q - 1, 2 q, the multiples of q next to 2^63 and 2^64, 2^64 - 1 and uniform words;
* the limit against its definition; the error draw against the restated sampler;
* the finish step c0 = Delta(m) - e - w at e = +-21 (and 0, +-1), w in {0, 1, q - 1}, Delta(m) at 0 and q - 1, and Delta_L(m) mod q_i as the
  kernel forms it at m = 0, 1, floor(t / 2), floor(t / 2) + 1, t - 1 against floor((q_L m + floor((t + 1) / 2)) / t).
No GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bfv_gpu_helpers as H
import bfv_seeded_ref as ref
import csim_lib

u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
U = C.c_uint64
GENERIC = 0x9e3779b97f4a7cd
SEED = 0xD1CE5EED


def declare(L):
    for name, res, args in (("sim_seeded_uniform", None, [U, U, u64p, U, U, u64p]), ("sim_seeded_error", None, [U, U, u64p, U, i32p]),
                            ("sim_seeded_limit", U, [U]), ("sim_seeded_reduce", U, [U, U]), ("sim_seeded_finish", U, [U, C.c_int, U, U]),
                            ("sim_seeded_delta", U, [u64p, C.c_int, U, U, C.c_int])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


@pytest.fixture(scope="module")
def chains():
    """{name: (moduli, t)} of every chain of ALL and of {45, 55, 50}: host-side contexts, no device"""
    be = importlib.import_module("reference-seal-backend_amd")
    out = {}
    for name, (N, bits, pb) in list(H.ALL.items()) + [("n2048_45_55_50", (2048, [45, 55, 50], 20))]:
        c = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
        out[name] = (list(c.moduli), c.t)
        c.close()
    return out


def core_uniform(sim, seed, stream, ns, q):
    ns = np.ascontiguousarray(ns, dtype=np.uint64)
    out = np.empty(len(ns), dtype=np.uint64)
    sim.sim_seeded_uniform(seed, stream, ns.ctypes.data_as(u64p), len(ns), q, out.ctypes.data_as(u64p))
    return out


def want_uniform(seed, stream, ns, q):
    v, draws = ref.uniform_draws(seed, stream, ns, q)
    return np.array([int(x) % q for x in v], dtype=np.uint64), draws


def test_uniform_draw_equals_percent_q(sim, chains):
    primes = sorted({q for moduli, _ in chains.values() for q in moduli} | {GENERIC})
    assert len(primes) >= 20 and {q.bit_length() for q in primes} >= {40, 45, 50, 55, 60}
    ns = np.arange(4096, dtype=np.uint64)
    for k, q in enumerate(primes):
        stream = ref.a_stream(1000 + k, k % 63)
        assert sim.sim_seeded_limit(q) == ref.limit(q) == (2 ** 64 // q) * q - 1
        want, _ = want_uniform(SEED, stream, ns, q)
        assert np.array_equal(core_uniform(sim, SEED, stream, ns, q), want), hex(q)
        assert int(want.max()) < q
        built = ref.seed_with_second_draw(stream, 4095, q, salt=k)
        want, draws = want_uniform(built, stream, ns, q)
        assert draws[4095] > 1 and np.array_equal(core_uniform(sim, built, stream, ns, q), want), hex(q)


def test_search_finds_second_draws_on_the_generic_prime(sim):
    q = GENERIC
    assert (2 ** 64 % q) * 2 ** 14 >= 2 ** 64, "rejection has probability >= 2^-14"
    stream = ref.a_stream(3, 0)
    ns = np.arange(1 << 20, dtype=np.uint64)
    want, draws = want_uniform(SEED, stream, ns, q)
    again = ns[draws > 1]
    assert len(again) > 1000 and (draws > 2).any()
    assert np.array_equal(core_uniform(sim, SEED, stream, again, q), want[draws > 1])


def test_barrett_reduction_is_exact_on_every_word(sim, chains):
    rng = np.random.default_rng(5)
    for q in sorted({q for moduli, _ in chains.values() for q in moduli} | {GENERIC}):
        k63, k64 = 2 ** 63 // q, 2 ** 64 // q
        edge = [0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, k63 * q - 1, k63 * q, k63 * q + 1, 2 ** 63 - 1, 2 ** 63, k64 * q - 1, k64 * q, 2 ** 64 - 1]
        for v in edge + [int(x) for x in rng.integers(0, 2 ** 64, 200, dtype=np.uint64)]:
            assert sim.sim_seeded_reduce(v, q) == v % q, (hex(q), v)


def test_error_draw(sim):
    ns = np.arange(4096, dtype=np.uint64)
    got = np.empty(4096, dtype=np.int32)
    stream = ref.e_stream((1 << 40) - 1)
    sim.sim_seeded_error(SEED, stream, ns.ctypes.data_as(u64p), 4096, got.ctypes.data_as(i32p))
    assert np.array_equal(got, ref.cbd(SEED, stream, 4096))


def test_finish_step(sim, chains):
    for q in sorted({q for moduli, _ in chains.values() for q in moduli}):
        for delta in (0, q - 1, 12345 % q):
            for e in (21, -21, 0, 1, -1):
                for w in (0, 1, q - 1):
                    assert sim.sim_seeded_finish(delta, e, w, q) == (delta - e - w) % q, (hex(q), delta, e, w)


def test_delta_as_the_kernel_forms_it(sim, chains):
    for name, (moduli, t) in chains.items():
        for L in sorted({1, len(moduli) - 1}):
            qs = moduli[:L]
            arr = (C.c_uint64 * L)(*qs)
            Q = int(np.prod([int(q) for q in qs], dtype=object))
            for m in (0, 1, t // 2, t // 2 + 1, t - 1):
                d = (Q * m + (t + 1) // 2) // t
                for i in range(L):
                    assert sim.sim_seeded_delta(arr, L, t, m, i) == d % qs[i], (name, L, m, i)
