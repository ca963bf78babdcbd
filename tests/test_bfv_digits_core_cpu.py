"""The arithmetic of the BFV ciphertext decomposition for recursive PIR on the CPU (tests/csim/sim_bfv_digits.cpp runs csrc/bfv_digits_core.h --
the digit table, a digit of a residue, the masked sum and its conditional subtraction, the functions the HIP kernels k_bfv_digits,
k_bfv_undigits and k_bfv_digits_cols_fwd compile -- and the centred lift of csrc/bfv_level_core.h the fused kernel applies to a digit), in
both builds of the u64 engine, against Python integers:

* the digit table: w = bitlen(t) - 1, D_i = ceil(b_i / w), off_i, F and the width of the top digit for t in {2, 3, 40961, 65537, 786433,
  1032193, 2^20, 2^20 + 7, 2^30 - 35} and b_i in {40, 45, 60}: exact division (60/20, 60/15, 45/15, everything by w = 1), non-exact
  division, the prime a digit index belongs to, and for every plaintext of a batch the (ciphertext, polynomial, prime, digit) the fused
  column pass cuts it from -- the inverse of "polynomial k, prime i, digit g of ciphertext r is plaintext r F + k D(L) + off_i + g";
* the digits of x in {0, 1, q - 1, floor(q / 2), 2^(g w) - 1, 2^(g w), 2^(g w) + 1 for every g} and uniform draws: every digit is below
  2^w <= t and sum digit 2^(g w) == x;
* compose: the identity on those digits; on arbitrary 64-bit "digits" the masked sum, reduced, in Python (q the smallest and a large value
  of its bit length: the sum is below 2^b < 2 q either way);
* the centred lift of digits at floor((t + 1) / 2) - 1, floor((t + 1) / 2) and 2^w - 1 under each prime: for t = 1032193 some digits lift
  negative, for t = 2^(w + 1) - 1 none do;
* the library without a device: the four entry points exist and are declared, he355_bfv_digit_count equals the Python table for the n1024
  and n4096_d3 chains, and a CKKS context, a bad L / L_out, size 0 / 4 and overlapping slabs are refused with HE355_E_INVALID_ARGS on the
  host, before any device is asked for (valid arguments then fail with HE355_E_DEVICE and touch nothing).
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

TS = [2, 3, 40961, 65537, 786433, 1032193, 2 ** 20, 2 ** 20 + 7, 2 ** 30 - 35]
BITS = [40, 45, 60]


def moduli_of(bits):
    """two stand-ins per bit length: the smallest odd value of that length (2^b < 2 q is tightest) and one just below 2^b"""
    return [(1 << (b - 1)) + 1 for b in bits], [(1 << b) - 93 for b in bits]


def py_table(qs, t):
    w = t.bit_length() - 1
    D = [-(-q.bit_length() // w) for q in qs]
    off = [sum(D[:i]) for i in range(len(qs) + 1)]
    return w, D, off


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfvdig_table.argtypes = [u64p, C.c_int, C.c_uint64, C.POINTER(C.c_int), u32p, u32p, u32p]
    L.sim_bfvdig_table.restype = C.c_uint32
    L.sim_bfvdig_keep.argtypes = [C.c_int] * 4
    L.sim_bfvdig_keep.restype = C.c_int
    L.sim_bfvdig_prime.argtypes = [u64p, C.c_int, C.c_uint64, C.c_uint32]
    L.sim_bfvdig_prime.restype = C.c_int
    L.sim_bfvdig_src.argtypes = [u64p, C.c_int, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.sim_bfvdig_src.restype = None
    L.sim_bfvdig_digits.argtypes = [C.c_uint64, C.c_int, C.c_int, u64p]
    L.sim_bfvdig_digits.restype = None
    L.sim_bfvdig_compose.argtypes = [u64p, C.c_int, C.c_int, C.c_int, C.c_uint64]
    L.sim_bfvdig_compose.restype = C.c_uint64
    L.sim_bfvdig_lift.argtypes = [C.c_uint64] * 3
    L.sim_bfvdig_lift.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def sim_table(sim, qs, t):
    L = len(qs)
    q = (C.c_uint64 * L)(*qs)
    w = C.c_int()
    D, off, bits = (C.c_uint32 * L)(), (C.c_uint32 * (L + 1))(), (C.c_uint32 * L)()
    total = sim.sim_bfvdig_table(q, L, t, C.byref(w), D, off, bits)
    return total, w.value, list(D), list(off), list(bits)


def test_digit_table(sim):
    seen = set()
    for t in TS:
        for qs in moduli_of(BITS) + moduli_of([60, 40, 40, 60, 45]):
            w, D, off = py_table(qs, t)
            assert 2 ** w <= t < 2 ** (w + 1)
            total, sw, sD, soff, sbits = sim_table(sim, qs, t)
            assert (sw, sD, soff, total) == (w, D, off, off[-1]), (t, qs)
            assert sbits == [q.bit_length() for q in qs]
            q = (C.c_uint64 * len(qs))(*qs)
            for i, b in enumerate(sbits):
                top = b - (D[i] - 1) * w
                assert 1 <= top <= w
                assert sim.sim_bfvdig_keep(D[i] - 1, D[i], b, w) == top
                assert all(sim.sim_bfvdig_keep(g, D[i], b, w) == w for g in range(D[i] - 1))
                for d in {off[i], off[i + 1] - 1}:  # first and last digit index of prime i
                    assert sim.sim_bfvdig_prime(q, len(qs), t, d) == i, (t, i, d)
                seen.add((b, w, b % w == 0))
            for size in (1, 2, 3):
                assert size * total == size * sum(D)  # F
    assert {(60, 20, True), (60, 15, True), (45, 15, True), (60, 1, True), (40, 1, True)} <= seen
    assert any(not exact for *_, exact in seen)


def test_source_of_every_plaintext(sim):
    for t in (3, 65537, 1032193, 2 ** 30 - 35):
        for qs in moduli_of(BITS) + moduli_of([60, 40, 40, 60, 45]):
            L = len(qs)
            w, D, off = py_table(qs, t)
            q = (C.c_uint64 * L)(*qs)
            out = (C.c_uint64 * 3)()
            for size in (1, 2, 3):
                F = size * off[-1]
                want = [(r, k, i, g) for r in range(3) for k in range(size) for i in range(L) for g in range(D[i])]
                assert len(want) == 3 * F
                for r, k, i, g in want:
                    pf = r * F + k * off[-1] + off[i] + g  # the definition
                    sim.sim_bfvdig_src(q, L, t, size, pf, out)
                    assert list(out) == [(r * size + k) * L + i, i, g], (t, qs, size, pf)


def digits_of(sim, x, D, w):
    out = (C.c_uint64 * D)()
    sim.sim_bfvdig_digits(x, D, w, out)
    return list(out)


def test_digits_and_identity(sim):
    rng = np.random.default_rng(71)
    for t in TS:
        w = t.bit_length() - 1
        for qs in moduli_of(BITS):
            for q in qs:
                b = q.bit_length()
                D = -(-b // w)
                xs = {0, 1, q - 1, q // 2} | {int(v) for v in rng.integers(0, q, 40, dtype=np.uint64)}
                for g in range(D):
                    xs |= {v for v in ((1 << (g * w)) - 1, 1 << (g * w), (1 << (g * w)) + 1) if v < q}
                for x in xs:
                    d = digits_of(sim, x, D, w)
                    assert all(v < 2 ** w <= t for v in d), (t, q, x)
                    assert sum(v << (g * w) for g, v in enumerate(d)) == x, (t, q, x)
                    assert sim.sim_bfvdig_compose((C.c_uint64 * D)(*d), D, b, w, q) == x, (t, q, x)


def test_compose_of_arbitrary_words(sim):
    rng = np.random.default_rng(72)
    for t in TS:
        w = t.bit_length() - 1
        for qs in moduli_of(BITS):
            for q in qs:
                b = q.bit_length()
                D = -(-b // w)
                top = b - (D - 1) * w
                cases = [[2 ** 64 - 1] * D, [0] * D] + [[int(v) for v in rng.integers(0, 2 ** 64, D, dtype=np.uint64)] for _ in range(30)]
                for d in cases:
                    s = sum((v & ((1 << (w if g + 1 < D else top)) - 1)) << (g * w) for g, v in enumerate(d))
                    assert s < 2 ** b < 2 * q
                    got = sim.sim_bfvdig_compose((C.c_uint64 * D)(*d), D, b, w, q)
                    assert got == s % q and got < q, (t, q, d)


def test_centred_lift_of_digits(sim, be):
    primes = set()
    for bits in ([60, 40, 60], [45, 45, 50, 60]):
        ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=bits, plain_bits=20, sec128=False)
        primes |= set(ctx.moduli)
        ctx.close()
    assert {40, 45, 60} <= {q.bit_length() for q in primes}
    for t in TS + [2 ** 20 - 1]:
        w = t.bit_length() - 1
        half = (t + 1) // 2
        digits = sorted({v for v in (0, 1, half - 1, half, 2 ** w - 1, 2 ** w // 2) if 0 <= v < 2 ** w})
        negative = 0
        for d in digits:
            c = d if d < half else d - t
            negative += c < 0
            for q in sorted(primes):
                assert sim.sim_bfvdig_lift(d, t, q) == c % q, (t, d, q)
        if t == 1032193:
            assert negative >= 2  # floor((t + 1) / 2) = 516097 < 2^19: the digits from there to 2^19 - 1 stand for negative coefficients
        if t == 2 ** (w + 1) - 1:
            assert negative == 0  # floor((t + 1) / 2) = 2^w: no w-bit digit reaches it


# ---- the library without a device ----------------------------------------------------------------------------------------------
NEW = ["he355_bfv_digit_count", "he355_bfv_decompose", "he355_bfv_decompose_ntt", "he355_bfv_compose"]
CHAINS = {"n1024": (1024, [50, 40, 50], 20), "n4096_d3": (4096, [60, 40, 40, 60], 20)}


@pytest.fixture(scope="module")
def newlib(be):
    lib = C.CDLL(be.LIB_PATH)
    for s in NEW:
        getattr(lib, s)  # AttributeError without the feature
    return be.lib()


def test_symbols_exported_and_declared(be, newlib):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_digit_count_equals_the_python_table(be, newlib, chain):
    N, bits, pb = CHAINS[chain]
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    for L in range(1, ctx.L + 1):
        w, D, off = py_table(ctx.moduli[:L], ctx.t)
        assert ctx.bfv_digit_count(L) == (off[-1], D), L
    assert ctx.bfv_digit_count(0) == (0, []) and ctx.bfv_digit_count(ctx.L + 1) == (0, [])
    buf = (C.c_uint32 * 2)(7, 7)  # cap: no more than cap entries are written, the count is still returned
    assert newlib.he355_bfv_digit_count(ctx.h, ctx.L, buf, 1) == sum(py_table(ctx.moduli[:ctx.L], ctx.t)[1]) and buf[1] == 7
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    assert ck.bfv_digit_count(1) == (0, [])
    ck.close()


def test_refusals_are_decided_on_the_host(be, newlib):
    N = 4096
    L = newlib
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    Lt = ctx.L
    F = 3 * ctx.bfv_digit_count(Lt)[0]
    ct = np.full(3 * Lt * N, 0xABCD, dtype=np.uint64)
    pl = np.full(F * Lt * N, 0xABCD, dtype=np.uint64)
    c, p = ct.ctypes.data_as(C.c_void_p), pl.ctypes.data_as(C.c_void_p)
    inside = C.c_void_p(p.value + 8 * N)  # a "ciphertext" that lies inside the plaintext slab
    bad = []
    for size in (0, 4):
        bad += [lambda s=size: L.he355_bfv_decompose(ctx.h, Lt, s, 1, c, p), lambda s=size: L.he355_bfv_compose(ctx.h, Lt, s, 1, p, c),
                lambda s=size: L.he355_bfv_decompose_ntt(ctx.h, Lt, s, 1, c, Lt, p)]
    for lv in (0, Lt + 1, -1):
        bad += [lambda v=lv: L.he355_bfv_decompose(ctx.h, v, 2, 1, c, p), lambda v=lv: L.he355_bfv_compose(ctx.h, v, 2, 1, p, c),
                lambda v=lv: L.he355_bfv_decompose_ntt(ctx.h, v, 2, 1, c, Lt, p), lambda v=lv: L.he355_bfv_decompose_ntt(ctx.h, Lt, 2, 1, c, v, p)]
    bad += [lambda: L.he355_bfv_decompose(ctx.h, 1, 1, 1, inside, p), lambda: L.he355_bfv_compose(ctx.h, 1, 1, 1, p, inside),
            lambda: L.he355_bfv_decompose_ntt(ctx.h, 1, 1, 1, inside, Lt, p), lambda: L.he355_bfv_decompose(ctx.h, Lt, 2, 2 ** 32, c, p)]
    for k, f in enumerate(bad):
        assert f() == be.E_INVALID_ARGS, k
        assert len(L.he355_last_error()) > 0
    # valid arguments: there is no device behind this context, and no CPU fallback
    assert L.he355_bfv_decompose(ctx.h, Lt, 3, 1, c, p) == be.E_DEVICE
    assert b"no CPU fallback" in L.he355_last_error()
    assert L.he355_bfv_decompose_ntt(ctx.h, 1, 2, 1, c, Lt, p) == be.E_DEVICE
    assert L.he355_bfv_compose(ctx.h, Lt, 3, 1, p, c) == be.E_DEVICE
    # the edge of the overlap rule, word for word: a ciphertext that starts in the last word of the plaintexts' range is refused, one
    # that starts right behind it is not.  The range is n F N words at the level's own F, times L_out for the NTT form.
    base = p.value
    at = lambda words: C.c_void_p(base + 8 * words)
    for lv in (1, Lt):
        per = 2 * ctx.bfv_digit_count(lv)[0] * N
        assert per * Lt + 2 * lv * N <= pl.size
        for f, end in ((lambda x: L.he355_bfv_decompose(ctx.h, lv, 2, 1, x, p), per), (lambda x: L.he355_bfv_compose(ctx.h, lv, 2, 1, p, x), per),
                       (lambda x: L.he355_bfv_decompose_ntt(ctx.h, lv, 2, 1, x, 1, p), per),
                       (lambda x: L.he355_bfv_decompose_ntt(ctx.h, lv, 2, 1, x, Lt, p), per * Lt)):
            assert f(at(end - 1)) == be.E_INVALID_ARGS, (lv, end)
            assert f(at(end - N)) == be.E_INVALID_ARGS, (lv, end)
            assert f(at(end)) == be.E_DEVICE, (lv, end)
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    for f in (lambda: L.he355_bfv_decompose(ck.h, ck.L, 2, 1, c, p), lambda: L.he355_bfv_decompose_ntt(ck.h, ck.L, 2, 1, c, ck.L, p),
              lambda: L.he355_bfv_compose(ck.h, ck.L, 2, 1, p, c)):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in L.he355_last_error()
    ck.close()
    assert (ct == 0xABCD).all() and (pl == 0xABCD).all()
