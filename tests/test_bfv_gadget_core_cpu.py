"""The arithmetic of the BFV external product on the CPU (tests/csim/sim_bfv_gadget.cpp runs csrc/bfv_gadget_core.h -- the width-v gadget
table, the uncentred digit under an output prime, the planted value of an RGSW row, the index maps of the fused column pass and the split of
a call into passes, the functions the HIP kernels of he355_kernels_bfv_gadget.hip compile), in both builds of the u64 engine, for EVERY digit
width v in 1..63, against Python integers over 35- to 60-bit moduli:

* the table: E_i = ceil(b_i / v), off_i, E(L); he355_bfv_gadget_count equals it for the n1024 and n4096_d3 chains at every level and width, and
  is 0 for a CKKS context, a bad level or a width outside 1..63;
* the digits of x in {0, 1, q - 1, floor(q / 2), 2^(g v) - 1, 2^(g v), 2^(g v) + 1 for every g} and uniform draws are the plain integers
  (x >> g v) & (2^v - 1), and the gadget identity sum digit G == x mod q_L holds for a 3-prime chain with the simulator's own digits and powers;
* the digit under an output prime: the identity below q_j, one reduction at or above it (v above the prime's bit length makes such digits);
* the planted value lift(m) 2^(g v) mod q_i at m in {0, 1, floor(t / 2), ceil(t / 2), t - 1} and every g;
* the index maps over a full batch (n size E odd included): digit polynomial -> (residue polynomial, prime, digit) is the stated order, and
  residue polynomial -> first digit polynomial, what a block of the column pass uses, is its inverse;
* the numpy reference of the GPU module (tests/bfv_gadget_ref.py) on small integers: digits, a digit above a 40-bit modulus, the identity, the
  negacyclic product by a sparse polynomial;
* the pass split: about 4096 digit polynomials, never fewer than one result, never more than n;
* the library without a device: the five entry points exist, are declared and bound; a CKKS context, a bad L, a bad v, size 0 / 4, inner == 0,
  inner 2 E above 2^31 - 1, a grid overflow, strides past 2^60 words and every overlap of the output with an input are refused with
  HE355_E_INVALID_ARGS and a message on the host, before any device is asked for (valid arguments then fail with HE355_E_DEVICE and touch
  nothing).  he355_bfv_rgsw_encrypt without a public key needs a device to hold no key: tests/test_gpu_bfv_external_product.py covers it.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import bfv_gadget_ref as ref
import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

WIDTHS = range(1, 64)
BITS = [35, 40, 45, 50, 60]
TS = [2, 3, 65537, 1032193, 2 ** 20, 2 ** 30 - 35]


def moduli_of(bits):
    """two stand-ins per bit length: the smallest odd value of that length and one just below 2^b"""
    return [(1 << (b - 1)) + 1 for b in bits], [(1 << b) - 93 for b in bits]


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfvgad_table.argtypes = [u64p, C.c_int, C.c_int, C.POINTER(C.c_int), u32p, u32p, u32p]
    L.sim_bfvgad_table.restype = C.c_uint32
    L.sim_bfvgad_width_ok.argtypes = [C.c_int]
    L.sim_bfvgad_width_ok.restype = C.c_int
    L.sim_bfvgad_digits.argtypes = [C.c_uint64, C.c_int, C.c_int, u64p]
    L.sim_bfvgad_digits.restype = None
    L.sim_bfvgad_digit_mod.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64]
    L.sim_bfvgad_digit_mod.restype = C.c_uint64
    L.sim_bfvgad_power.argtypes = [C.c_int, C.c_int]
    L.sim_bfvgad_power.restype = C.c_uint64
    L.sim_bfvgad_plant.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64]
    L.sim_bfvgad_plant.restype = C.c_uint64
    L.sim_bfvgad_src.argtypes = [u64p, C.c_int, C.c_int, C.c_int, C.c_uint64, u64p]
    L.sim_bfvgad_src.restype = None
    L.sim_bfvgad_first.argtypes = [u64p, C.c_int, C.c_int, C.c_int, C.c_uint64]
    L.sim_bfvgad_first.restype = C.c_uint64
    L.sim_bfvgad_pass.argtypes = [C.c_uint64] * 3
    L.sim_bfvgad_pass.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def sim_table(sim, qs, v):
    L = len(qs)
    q = (C.c_uint64 * L)(*qs)
    w = C.c_int()
    E, off, bits = (C.c_uint32 * L)(), (C.c_uint32 * (L + 1))(), (C.c_uint32 * L)()
    total = sim.sim_bfvgad_table(q, L, v, C.byref(w), E, off, bits)
    return total, w.value, list(E), list(off), list(bits)


def test_gadget_table_every_width(sim):
    assert [v for v in range(-1, 66) if sim.sim_bfvgad_width_ok(v)] == list(WIDTHS)
    single = 0
    for v in WIDTHS:
        for qs in moduli_of(BITS) + moduli_of([60, 40, 60]):
            E, off = ref.table(qs, v)
            total, w, sE, soff, sbits = sim_table(sim, qs, v)
            assert (w, sE, soff, total) == (v, E, off, off[-1]), (v, qs)
            assert sbits == [q.bit_length() for q in qs]
            for e, b in zip(E, sbits):
                assert (e - 1) * v < b <= e * v  # every shift g v is below the prime's bit length, and the digits cover it
            single += all(e == 1 for e in E)
    assert single  # v >= 60: one digit per prime


def digits_of(sim, x, E, v):
    out = (C.c_uint64 * E)()
    sim.sim_bfvgad_digits(x, E, v, out)
    return list(out)


def test_digits_are_plain_integers_and_the_gadget_identity(sim):
    rng = np.random.default_rng(81)
    for v in WIDTHS:
        for qs in moduli_of([60, 40, 35]) + moduli_of([45, 50, 60]):
            E, off = ref.table(qs, v)
            values = []
            for q, e in zip(qs, E):
                xs = [0, 1, q - 1, q // 2] + [int(x) for x in rng.integers(0, q, 6, dtype=np.uint64)]
                for g in range(e):
                    xs += [x for x in ((1 << (g * v)) - 1, 1 << (g * v), (1 << (g * v)) + 1) if x < q]
                for x in xs:
                    d = digits_of(sim, x, e, v)
                    assert d == [ref.digit(x, g, v) for g in range(e)], (v, q, x)
                    assert all(0 <= y < 2 ** v for y in d) and sum(y << (g * v) for g, y in enumerate(d)) == x
                values.append(xs)
            # the identity mod q_L with the simulator's digits and powers: G_(i,g) = 2^(g v) under prime i, 0 under the others
            for k in range(8):
                x = [vals[k % len(vals)] for vals in values]
                for j, qj in enumerate(qs):
                    s = sum(y * (sim.sim_bfvgad_power(g, v) % qs[i] if i == j else 0)
                            for i in range(len(qs)) for g, y in enumerate(digits_of(sim, x[i], E[i], v)))
                    assert s % qj == x[j], (v, qs, x, j)
                assert ref.identity_holds(x, qs, v)
            for i, q in enumerate(qs):
                for g in range(E[i]):
                    assert sim.sim_bfvgad_power(g, v) == 1 << (g * v) < q  # canonical under its own prime as it stands


def test_digit_under_an_output_prime(sim):
    rng = np.random.default_rng(82)
    reduced = set()
    for v in WIDTHS:
        for qs in moduli_of(BITS):
            for qi in qs:  # the prime the residue lives under
                e = -(-qi.bit_length() // v)
                xs = [0, 1, qi - 1, qi // 2] + [int(x) for x in rng.integers(0, qi, 4, dtype=np.uint64)]
                for qj in qs:  # the output prime
                    for x in xs:
                        for g in range(e):
                            d = ref.digit(x, g, v)
                            assert sim.sim_bfvgad_digit_mod(x, g, v, qj) == d % qj, (v, qi, qj, x, g)
                            if d >= qj:
                                reduced.add(v)
    # a digit reaches an output prime only where 2^v is above it: v = 45 against the 35- and 40-bit moduli is such a width
    assert 45 in reduced and min(reduced) >= 35 and not reduced & set(range(1, 35))


def test_planted_value(sim):
    for v in WIDTHS:
        for qs in moduli_of(BITS):
            for q in qs:
                for t in TS:
                    for m in sorted({0, 1 % t, t // 2, (t + 1) // 2, t - 1}):
                        for g in range(-(-q.bit_length() // v)):
                            assert sim.sim_bfvgad_plant(m, t, g, v, q) == ref.plant(m, t, g, v, q), (v, q, t, m, g)
    assert ref.plant(2, 3, 1, 4, 97) == (97 - 16) and ref.plant(1, 3, 1, 4, 97) == 16  # t - 1 plants -2^(g v)


def test_index_maps_of_the_column_pass(sim):
    odd = 0
    for v in (1, 4, 20, 45, 63):
        for qs in moduli_of([60, 40, 35]) + moduli_of([60, 40, 40, 60, 45]):
            L = len(qs)
            E, off = ref.table(qs, v)
            q = (C.c_uint64 * L)(*qs)
            out = (C.c_uint64 * 3)()
            for size in (1, 2, 3):
                n = 3
                total = n * size * off[-1]
                odd += total % 2
                want = [(c, k, i, g) for c in range(n) for k in range(size) for i in range(L) for g in range(E[i])]
                assert len(want) == total
                for pf, (c, k, i, g) in enumerate(want):
                    assert pf == c * size * off[-1] + k * off[-1] + off[i] + g  # the definition's order
                    sim.sim_bfvgad_src(q, L, v, size, pf, out)
                    p = (c * size + k) * L + i
                    assert list(out) == [p, i, g], (v, qs, size, pf)
                    assert sim.sim_bfvgad_first(q, L, v, size, p) == pf - g
                # the blocks of the column pass tile the digit polynomials: every residue polynomial's E_i follow the one before
                nxt = 0
                for p in range(n * size * L):
                    assert sim.sim_bfvgad_first(q, L, v, size, p) == nxt
                    nxt += E[p % L]
                assert nxt == total
    assert odd


def test_pass_split(sim):
    for terms in (2, 10, 30, 270, 4095, 4096, 4097, 10 ** 6):
        for n in (1, 2, 3, 64, 1024, 10 ** 6):
            p = sim.sim_bfvgad_pass(terms, n, 4096)
            assert 1 <= p <= n
            assert p == max(1, min(n, 4096 // terms))
            assert p * terms <= 4096 or p == 1  # at most the cap, unless one result alone is more


def test_np_reference_on_small_integers():
    q, v = [(1 << 60) - 93, (1 << 39) + 1], 45
    E, off = ref.table(q, v)
    assert (E, off) == ([2, 1], [0, 2, 3])
    x = np.array([[0, 1, q[0] - 1, (1 << 45) + 5], [5, (1 << 38) + 7, q[1] - 1, 1 << 19]], dtype=np.uint64).reshape(1, 1, 2, 4)
    d = ref.np_digits(x, q, v)
    assert d.shape == (1, 3, 4) and int(d[0, 0, 2]) == (q[0] - 1) & ((1 << 45) - 1) >= q[1]  # a digit above the 40-bit modulus
    assert int(ref.np_spread(d, q)[0, 0, 1, 2]) == int(d[0, 0, 2]) % q[1]
    for e in range(4):
        assert ref.identity_holds([int(x[0, 0, 0, e]), int(x[0, 0, 1, e])], q, v)
    mu = np.array([1, 2, 3, 4], dtype=np.uint64)
    assert list(ref.negacyclic_sparse(mu, {1: 1}, 17)) == [13, 1, 2, 3] and list(ref.negacyclic_sparse(mu, {0: 16}, 17)) == [16, 15, 14, 13]


# ---- the library without a device ----------------------------------------------------------------------------------------------
NEW = ["he355_bfv_gadget_count", "he355_bfv_gadget_decompose", "he355_bfv_gadget_decompose_ntt", "he355_bfv_rgsw_encrypt", "he355_bfv_external_product"]
CHAINS = {"n1024": (1024, [50, 40, 50], 20), "n4096_d3": (4096, [60, 40, 40, 60], 20)}


@pytest.fixture(scope="module")
def newlib(be):
    lib = C.CDLL(be.LIB_PATH)
    for s in NEW:
        getattr(lib, s)  # AttributeError without the feature
    return be.lib()


def test_symbols_exported_declared_and_bound(be, newlib):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_gadget_count_equals_the_python_table(be, newlib, chain):
    N, bits, pb = CHAINS[chain]
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    for L in range(1, ctx.L + 1):
        for v in WIDTHS:
            E, off = ref.table(ctx.moduli[:L], v)
            assert ctx.bfv_gadget_count(L, v) == (off[-1], E), (L, v)
    for L, v in ((0, 20), (ctx.L + 1, 20), (-1, 20), (1, 0), (1, 64), (1, -3)):
        assert ctx.bfv_gadget_count(L, v) == (0, [])
    buf = (C.c_uint32 * 2)(7, 7)  # cap: no more than cap entries are written, the count is still returned
    assert newlib.he355_bfv_gadget_count(ctx.h, ctx.L, 20, buf, 1) == ref.table(ctx.moduli[:ctx.L], 20)[1][-1] and buf[1] == 7
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    assert ck.bfv_gadget_count(1, 20) == (0, [])
    ck.close()


def test_refusals_are_decided_on_the_host(be, newlib):
    N, v = 4096, 20
    lib = newlib
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    Lt = ctx.L
    E = ctx.bfv_gadget_count(Lt, v)[0]
    per = 2 * Lt * N
    a = np.full(4 * per, 0xABCD, dtype=np.uint64)                 # ciphertexts / plaintexts
    b = np.full(3 * E * Lt * N + 2 * E * per, 0xABCD, dtype=np.uint64)  # digits / RGSW rows / results
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    at = lambda base, words: C.c_void_p(base.value + 8 * words)
    dec = lambda L=Lt, w=v, size=2, n=1, src=pa, dst=pb: lib.he355_bfv_gadget_decompose(ctx.h, L, w, size, n, src, dst)
    ntt = lambda L=Lt, w=v, size=2, n=1, src=pa, dst=pb: lib.he355_bfv_gadget_decompose_ntt(ctx.h, L, w, size, n, src, dst)
    enc = lambda L=Lt, w=v, n=1, src=pa, dst=pb: lib.he355_bfv_rgsw_encrypt(ctx.h, L, w, n, src, 1, 0, dst)
    # external product: the ciphertexts in a, the RGSW in b, the output behind the RGSW
    out = at(pb, 2 * E * per - per)  # overlaps the last row of the RGSW on purpose in `ep_bad`; `ep` puts it into a
    ep = lambda L=Lt, w=v, n=1, inner=1, ct=at(pa, per), sr=1, sk=1, rg=pb, gr=0, gk=1, dst=pa: \
        lib.he355_bfv_external_product(ctx.h, L, w, n, inner, ct, sr, sk, rg, gr, gk, dst)
    bad = []
    for f in (dec, ntt, enc, ep):
        bad += [lambda f=f: f(L=0), lambda f=f: f(L=Lt + 1), lambda f=f: f(L=-1), lambda f=f: f(w=0), lambda f=f: f(w=64), lambda f=f: f(w=-1)]
    for f in (dec, ntt):
        bad += [lambda f=f: f(size=0), lambda f=f: f(size=4), lambda f=f: f(n=2 ** 32),            # n size E above 2^32 - 1
                lambda f=f: f(n=2 ** 28, w=63),                                                    # the grid of one launch
                lambda f=f: f(src=pb), lambda f=f: f(src=at(pb, N))]                               # the same slab; the input inside the output
    bad += [lambda: enc(src=pb), lambda: enc(src=at(pb, 2 * E * per - N)), lambda: enc(n=2 ** 31)]
    bad += [lambda: ep(inner=0), lambda: ep(inner=2 ** 31 // (2 * E) + 1), lambda: ep(inner=2 ** 62),  # inner 2E above 2^31 - 1 (and a wrap)
            lambda: ep(n=2 ** 31), lambda: ep(n=2 ** 29, w=63),                                      # the grid
            lambda: ep(n=2, sr=2 ** 50), lambda: ep(n=2, gr=2 ** 63), lambda: ep(inner=2, sk=2 ** 60),  # strides that cannot be indices
            lambda: ep(dst=at(pa, per)), lambda: ep(dst=at(pa, 2 * per - 1)),                        # the output on / inside the ciphertext
            lambda: ep(n=2, inner=1, ct=at(pa, 2 * per), sr=1, dst=at(pa, per - 1 + per)),           # ... inside the second result's ciphertext
            lambda: ep(dst=out), lambda: ep(dst=pb),                                                  # the output inside the RGSW rows
            lambda: ep(n=2, gr=1, rg=pb, dst=at(pb, 2 * E * per)),                                    # gr = 1: the second selector row is read too
            lambda: ep(inner=2, ct=pa, sk=3, dst=at(pa, 3 * per))]                                    # ciphertext (0, 1) at stride 3
    for k, f in enumerate(bad):
        assert f() == be.E_INVALID_ARGS, k
        assert len(lib.he355_last_error()) > 0, k
    # valid arguments: there is no device behind this context, and no CPU fallback
    for f in (lambda: dec(size=3, n=1), lambda: ntt(size=3), lambda: ntt(L=1), lambda: enc(), lambda: enc(L=1), lambda: ep(), lambda: ep(L=1, w=63),
              lambda: ep(n=2, inner=1, ct=at(pa, 2 * per), dst=pa), lambda: ep(dst=at(pb, 2 * E * per)),  # right behind the one selector row
              lambda: ep(inner=2, ct=pa, sk=2, dst=at(pa, 3 * per))):                                   # right behind ciphertext (0, 1)
        assert f() == be.E_DEVICE
        assert b"no CPU fallback" in lib.he355_last_error()
    # n == 0 is still an argument check away from the device
    assert ep(n=0, inner=0) == be.E_INVALID_ARGS and ep(n=0) == be.E_DEVICE
    # the edge of the overlap rule of the cut, word for word
    for lv in (1, Lt):
        e = ctx.bfv_gadget_count(lv, v)[0]
        for f, end in ((lambda x: dec(L=lv, src=x), 2 * e * N), (lambda x: ntt(L=lv, src=x), 2 * e * lv * N)):
            assert f(at(pb, end - 1)) == be.E_INVALID_ARGS, (lv, end)
            assert f(at(pb, end)) == be.E_DEVICE, (lv, end)
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    for f in (lambda: lib.he355_bfv_gadget_decompose(ck.h, 1, v, 2, 1, pa, pb), lambda: lib.he355_bfv_gadget_decompose_ntt(ck.h, 1, v, 2, 1, pa, pb),
              lambda: lib.he355_bfv_rgsw_encrypt(ck.h, 1, v, 1, pa, 1, 0, pb),
              lambda: lib.he355_bfv_external_product(ck.h, 1, v, 1, 1, pa, 1, 1, pb, 0, 1, at(pa, per))):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (a == 0xABCD).all() and (b == 0xABCD).all()
