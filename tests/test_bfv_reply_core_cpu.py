"""The arithmetic of BFV reply compression on the CPU (tests/csim/sim_bfv_reply.cpp runs csrc/bfv_reply_core.h -- the functions the HIP kernels
k_bfv_reply_pack, k_bfv_reply_lift and k_bfv_reply_finish compile) against the definition in Python integers (tests/bfv_reply_ref.py), in
both builds of the u64 engine, under a 60-, a 50-, a 40- and a 35-bit prime, for every width k in 2..46 the prime accepts at N = 1024:

* the switch at x = 0, 1, floor(q / 2), floor(q / 2) + 1, q - 1; at the rounding boundaries of 64 sampled y plus y = 1 and y = 2^k - 1 -- the
  smallest x that rounds to y, ceil((2 y - 1) q / 2^(k + 1)), and the x below it; at the smallest x that rounds to 2^k, which wraps to 0, and
  the x below it; and at uniform x; the word rule's division by k at every bit position a half of N = 1024, and the end of a half of N = 32768, has on a
  word's first and last bit;
* packing and extraction at N = 128 and 1024: all-ones fields, alternating all-ones / zero fields, uniform fields (fields that end on bit 63
  and start on bit 0 are among them whenever k does not divide 64), the last field of c0 and the first of c1 all ones next to zero
  neighbours: the two halves' words, joined, are the reference's bytes, and extraction returns the fields;
* the centred lift at 0, 1, 2^(k1 - 1) - 1, 2^(k1 - 1), 2^k1 - 1;
* the final rounding: z on both sides of every tie for sampled M, z = 0 and 2^k1 - 1, and the z that round to M = t, which reduces to 0;
  each z split into (y0, w) with w positive and, where k1 > k0, with w negative (q - ..): plaintext and residue bit length;
* widths, sizes and the safe pair against the reference.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import bfv_reply_ref as ref
import csim_lib

u64p = C.POINTER(C.c_uint64)
PRIMES = {60: 0xfffffffffff2801, 50: 0x3ffffffffa801, 40: 0xffffff7801, 35: 0x7ffffc801}
T = 1038337
KS = range(2, 47)


def declare(L):
    L.sim_bfvreply_widths_ok.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    L.sim_bfvreply_widths_ok.restype = C.c_int
    L.sim_bfvreply_size.argtypes = [C.c_uint64, C.c_int, C.c_int]
    L.sim_bfvreply_size.restype = C.c_uint64
    L.sim_bfvreply_safe.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sim_bfvreply_safe.restype = None
    L.sim_bfvreply_div.argtypes = [C.c_uint32, C.c_int]
    L.sim_bfvreply_div.restype = C.c_uint32
    L.sim_bfvreply_cut.argtypes = [u64p, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.sim_bfvreply_cut.restype = None
    L.sim_bfvreply_pack.argtypes = [u64p, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.sim_bfvreply_pack.restype = None
    L.sim_bfvreply_unpack.argtypes = [u64p, C.c_uint64, C.c_int, u64p]
    L.sim_bfvreply_unpack.restype = None
    L.sim_bfvreply_lift.argtypes = [C.c_uint64, C.c_int, C.c_uint64]
    L.sim_bfvreply_lift.restype = C.c_uint64
    L.sim_bfvreply_round.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]
    L.sim_bfvreply_round.restype = C.c_uint64
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def widths(q, N=1024):
    return [k for k in KS if ref.accepted(N, q, 2, k)]


def smallest_rounding_to(y, k, q):
    return -(-(2 * y - 1) * q // 2 ** (k + 1))


def cuts(sim, xs, k, q):
    a = (C.c_uint64 * len(xs))(*xs)
    out = (C.c_uint64 * len(xs))()
    sim.sim_bfvreply_cut(a, len(xs), k, q, out)
    return list(out)


def test_every_width_is_covered_by_some_prime():
    assert widths(PRIMES[60]) == list(KS) and widths(PRIMES[50])[-1] == 39 and widths(PRIMES[40])[-1] == 29 and widths(PRIMES[35])[-1] == 24


@pytest.mark.parametrize("bits", sorted(PRIMES))
def test_switch(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(900 + bits)
    for k in widths(q):
        ys = sorted({1, 2 ** k - 1} | {int(y) for y in rng.integers(1, 2 ** k, 64)})
        xs = [0, 1, q // 2, q // 2 + 1, q - 1]
        for y in ys:
            x = smallest_rounding_to(y, k, q)
            assert 0 < x < q and ref.cut(x, k, q) == y and ref.cut(x - 1, k, q) == y - 1, (k, y)
            xs += [x, x - 1]
        wrap = smallest_rounding_to(2 ** k, k, q)
        assert wrap < q and ref.cut(wrap, k, q) == 0 and ref.cut(wrap - 1, k, q) == 2 ** k - 1
        xs += [wrap, wrap - 1]
        xs += [int(x) for x in rng.integers(0, q, 64, dtype=np.uint64)]
        assert cuts(sim, xs, k, q) == [ref.cut(x, k, q) for x in xs], (bits, k)


def test_division_by_the_width(sim):
    for k in range(2, 63):
        top = 32768 * k
        for p in list(range(0, 1024 * k, 64)) + list(range(63, 1024 * k, 64)) + list(range(top - 4096, top, 64)) + list(range(top - 4033, top, 64)):
            assert sim.sim_bfvreply_div(p, k) == p // k, (k, p)


def field_sets(rng, N, k):
    ones = 2 ** k - 1
    yield "ones", [ones] * N
    yield "alternating", [ones if e % 2 == 0 else 0 for e in range(N)]
    yield "alternating'", [0 if e % 2 == 0 else ones for e in range(N)]
    yield "uniform", [int(v) for v in rng.integers(0, 2 ** k, N, dtype=np.uint64)]
    yield "first", [ones] + [0] * (N - 1)
    yield "last", [0] * (N - 1) + [ones]


@pytest.mark.parametrize("bits", sorted(PRIMES))
def test_packing_and_extraction(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(901 + bits)
    for N in (128, 1024):
        ks = widths(q, N) if N == 1024 else widths(q)
        for k in ks if N == 128 else ks[::7] + ks[-1:]:
            # fields that end on bit 63 / start on bit 0 inside the half: e k = 0 (mod 64)
            assert any((e * k) % 64 == 0 for e in range(1, N))
            W = N * k // 64
            for name, y in field_sets(rng, N, k):
                coef = [smallest_rounding_to(v, k, q) if v else 0 for v in y]
                words = (C.c_uint64 * W)()
                sim.sim_bfvreply_pack((C.c_uint64 * N)(*coef), N, k, q, words)
                # the half as c0 in front of an all-zero c1 of the same width, and as c1 behind an all-zero c0: the reference's bytes
                as_c0 = ref.pack(y, [0] * N, k, k)
                as_c1 = ref.pack([0] * N, y, k, k)
                got = bytes(words)
                assert got == as_c0[:8 * W] and got == as_c1[8 * W:], (bits, N, k, name)
                out = (C.c_uint64 * N)()
                sim.sim_bfvreply_unpack(words, N, k, out)
                assert list(out) == y, (bits, N, k, name)


def test_two_halves_make_the_reference_reply(sim):
    """the last field of c0 and the first of c1, with different widths"""
    q, N = PRIMES[60], 128
    rng = np.random.default_rng(902)
    for k0, k1 in ((2, 2), (22, 32), (22, 35), (31, 33), (3, 46), (46, 46)):
        for y0, y1 in (([0] * (N - 1) + [2 ** k0 - 1], [0] * N), ([0] * N, [2 ** k1 - 1] + [0] * (N - 1)),
                       ([int(v) for v in rng.integers(0, 2 ** k0, N)], [int(v) for v in rng.integers(0, 2 ** k1, N)])):
            data = b""
            for y, k in ((y0, k0), (y1, k1)):
                coef = [smallest_rounding_to(v, k, q) if v else 0 for v in y]
                words = (C.c_uint64 * (N * k // 64))()
                sim.sim_bfvreply_pack((C.c_uint64 * N)(*coef), N, k, q, words)
                data += bytes(words)
            assert data == ref.pack(y0, y1, k0, k1) and len(data) == sim.sim_bfvreply_size(N, k0, k1)
            assert data == ref.compress([smallest_rounding_to(v, k0, q) if v else 0 for v in y0], [smallest_rounding_to(v, k1, q) if v else 0 for v in y1], q, k0, k1)


@pytest.mark.parametrize("bits", sorted(PRIMES))
def test_centred_lift(sim, bits):
    q = PRIMES[bits]
    for k1 in widths(q):
        for y in sorted({0, 1, 2 ** (k1 - 1) - 1, 2 ** (k1 - 1), 2 ** k1 - 1}):
            assert sim.sim_bfvreply_lift(y, k1, q) == ref.centre(y, k1) % q, (bits, k1, y)


@pytest.mark.parametrize("bits", sorted(PRIMES))
def test_final_rounding(sim, bits):
    q = PRIMES[bits]
    rng = np.random.default_rng(903 + bits)
    nb = C.c_int(0)
    for t in (T, 2, 65537, 2 ** 20):
        for k1 in widths(q):
            for k0 in sorted({2, k1 // 2 + 1, k1} & set(range(2, k1 + 1))):
                Ms = sorted({1, t} | {int(m) for m in rng.integers(1, t + 1, 6)})
                zs = {0, 2 ** k1 - 1}
                for M in Ms:  # the smallest z that rounds to M, and the z below it
                    z = -(-(2 * M - 1) * 2 ** (k1 - 1) // t)
                    if z < 2 ** k1:
                        if t <= 2 ** k1:  # (a step of z then moves M by at most one)
                            assert (t * z + 2 ** (k1 - 1)) // 2 ** k1 == M and (t * (z - 1) + 2 ** (k1 - 1)) // 2 ** k1 == M - 1
                        zs |= {z, z - 1}
                sh = k1 - k0
                for z in sorted(zs):
                    splits = [(z >> sh, z & (2 ** sh - 1))]
                    if sh and z & (2 ** sh - 1):
                        splits.append((((z >> sh) + 1) % 2 ** k0, (z & (2 ** sh - 1)) - 2 ** sh))  # the same z from a negative product
                    for y0, w in splits:
                        want, r = ref.finish([y0], [w], k0, k1, t)
                        got = sim.sim_bfvreply_round(y0, w % q, k0, k1, q, t, C.byref(nb))
                        assert (got, nb.value) == (want[0], r.bit_length()), (bits, t, k0, k1, z, y0, w)
                z = 2 ** k1 - 1  # M = t (reached whenever 2^(k1 - 1) >= t) reduces to 0
                if (t * z + 2 ** (k1 - 1)) // 2 ** k1 == t:
                    assert sim.sim_bfvreply_round(z >> sh, z & (2 ** sh - 1), k0, k1, q, t, C.byref(nb)) == 0


def test_widths_sizes_and_the_safe_pair(sim):
    k0, k1 = C.c_int(0), C.c_int(0)
    for N in (1024, 4096, 8192, 32768):
        for t in (T, 786433, 65537, 2, 2 ** 20):
            sim.sim_bfvreply_safe(N, t, C.byref(k0), C.byref(k1))
            assert (k0.value, k1.value) == ref.safe_bits(N, t)
        for q in PRIMES.values():
            top = ref.max_width(N, q) if ref.accepted(N, q, 2, 2) else 1
            for a, b in ((2, 2), (1, 2), (0, 5), (-1, 5), (3, 2), (2, top), (top, top), (2, top + 1), (top + 1, top + 1), (22, 32), (2, 63), (2, 64), (2, 200)):
                assert bool(sim.sim_bfvreply_widths_ok(N, q, a, b)) == ref.accepted(N, q, a, b), (N, q, a, b)
        assert sim.sim_bfvreply_size(N, 22, 35) == ref.reply_bytes(N, 22, 35)
    assert sim.sim_bfvreply_size(8192, 22, 35) == 58368 and sim.sim_bfvreply_size(32768, 22, 37) == 241664
