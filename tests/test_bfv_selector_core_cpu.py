"""The arithmetic of the packed RGSW selectors on the CPU (tests/csim/sim_bfv_selector.cpp runs csrc/bfv_gadget_core.h -- (2^d)^(-1) mod q, the
value a selector plants and the destination row of a slot ciphertext, the functions the HIP kernels of he355_bfv_selector_encrypt and
he355_bfv_rgsw_from_bfv compile), in both builds of the u64 engine, against Python integers.  Exact: no tolerance.

* the planted value lift(m) 2^(g v) (2^d)^(-1) mod q_i: m in {0, 1, t - 1, floor(t / 2), floor((t + 1) / 2)}, every (i, g) of the gadget tables
  for v in {4, 20, 45, 63} on the chains n1024, (2048, {60, 40, 60}, 20) and n4096_d3 at L in {L_top, 1}, d in {0, 1, log2 N}; (2^d)^(-1) 2^d == 1;
* the row rule over two selectors: the k = 0 rows then the k = 1 rows of selector 0, then selector 1's, every row taken once;
* the numpy reference's packing (tests/bfv_selector_ref.py) against a by-hand expansion of one slot: multiply by 2^d and read the coefficient;
  every other word is the encryption of zero's;
* the library without a device: the three entry points exist, are declared and bound; every refusal that needs no device is decided on the host
  with HE355_E_INVALID_ARGS and a message (valid arguments then fail with HE355_E_DEVICE and touch nothing).  The missing-key refusals need a
  device to hold no key: tests/test_gpu_bfv_selectors.py covers them.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import bfv_gadget_ref as gad
import bfv_selector_ref as ref
import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHAINS = {"n1024": (1024, [50, 40, 50], 20), "n2048": (2048, [60, 40, 60], 20), "n4096_d3": (4096, [60, 40, 40, 60], 20),
          "n1024_f64_first": (1024, [45, 55, 50], 20)}  # the last: an fp64 prime 0 beside a u64 one (test_gpu_bfv_chain_layouts.py)
WIDTHS = (4, 20, 45, 63)
NEW = ["he355_bfv_selector_encrypt", "he355_bfv_rgsw_encrypt_secret", "he355_bfv_rgsw_from_bfv"]


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfv_selector_inv_pow2.argtypes = [C.c_uint64, C.c_int]
    L.sim_bfv_selector_inv_pow2.restype = C.c_uint64
    L.sim_bfv_selector_value.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64]
    L.sim_bfv_selector_value.restype = C.c_uint64
    L.sim_bfv_selector_row.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
    L.sim_bfv_selector_row.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


@pytest.fixture(scope="module")
def chains(be):
    """name -> (N, the data primes, t), from the library's own parameter search (host side, no device)"""
    out = {}
    for name, (N, bits, pb) in CHAINS.items():
        ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
        out[name] = (N, list(ctx.moduli[:ctx.L]), ctx.t)
        ctx.close()
    return out


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_planted_selector_value(sim, chains, chain):
    N, moduli, t = chains[chain]
    checked = 0
    for L in sorted({len(moduli), 1}):
        for v in WIDTHS:
            E, _ = gad.table(moduli[:L], v)
            for d in (0, 1, N.bit_length() - 1):
                for i, q in enumerate(moduli[:L]):
                    inv = sim.sim_bfv_selector_inv_pow2(q, d)
                    assert 0 < inv < q and inv * (1 << d) % q == 1, (q, d)
                    for g in range(E[i]):
                        for m in sorted({0, 1, t - 1, t // 2, (t + 1) // 2}):
                            lifted = m if m < (t + 1) // 2 else m - t
                            want = lifted * 2 ** (g * v) * pow(2 ** d, -1, q) % q
                            assert ref.value(m, t, g, v, d, q) == want
                            assert sim.sim_bfv_selector_value(m, t, g, v, d, q) == want, (L, v, d, q, g, m)
                            assert want * 2 ** d % q == lifted * 2 ** (g * v) % q  # the expansion's 2^d gives lift(m) G_(i,g) back
                            checked += 1
    assert checked >= 5 * 3 * 4 * 2


def test_row_rule_over_two_selectors(sim):
    for E in (1, 2, 3, 7, 15, 35):
        rows = []
        for c in range(2 * E):
            for k in (0, 1):
                r = sim.sim_bfv_selector_row(c, E, k)
                assert r == ref.row(c, E, k) == (c // E) * 2 * E + k * E + c % E, (E, c, k)
                rows.append((r, c // E, k, c % E))
        # selector 0's k = 0 rows, its k = 1 rows, then selector 1's: row = b 2E + k E + f, every row of the two RGSW ciphertexts once
        assert sorted(r for r, *_ in rows) == list(range(4 * E))
        for r, b, k, f in rows:
            assert (r // (2 * E), (r % (2 * E)) // E, r % E) == (b, k, f)
    # far into a batch: no 32-bit wrap
    assert sim.sim_bfv_selector_row(2 ** 40 + 3, 7, 1) == ((2 ** 40 + 3) // 7) * 14 + 7 + (2 ** 40 + 3) % 7


def test_np_packing_against_a_by_hand_expansion():
    rng = np.random.default_rng(91)
    moduli, t, N = [(1 << 60) - 93, (1 << 39) + 7, (1 << 40) - 87], 1032193, 64
    for L in (3, 1):
        for v, n_sel, first_slot, count in ((20, 3, 5, 64), (20, 2, 0, 14 if L == 3 else 6), (45, 4, 8, 32), (63, 1, 0, L)):
            E, off = gad.table(moduli[:L], v)
            assert first_slot + n_sel * off[-1] <= count
            d = ref.depth(count)
            assert 2 ** d >= count > (2 ** d) // 2
            zero = np.stack([[[rng.integers(0, q, N, dtype=np.uint64) for q in moduli[:L]] for _ in range(2)] for _ in range(2)])
            sel = rng.integers(0, t, (2, n_sel), dtype=np.uint64)
            sel[0, 0] = t - 1
            sel[1, -1] = 0
            got = ref.np_pack(zero, sel, moduli, t, v, first_slot, count)
            touched = np.zeros(got.shape, dtype=bool)
            where = ref.slots(moduli[:L], v, n_sel, first_slot)
            assert [e for e, *_ in where] == list(range(first_slot, first_slot + n_sel * off[-1]))  # the slots follow one another
            for r in range(2):
                for e, b, i, g in where:
                    assert e == first_slot + b * off[-1] + off[i] + g
                    for j, q in enumerate(moduli[:L]):
                        # the phase the packing adds, after the expansion's 2^d: lift(m) G_(i,g), i.e. 2^(g v) under prime i and 0 elsewhere
                        added = (ref.expanded_constant(got[r, 0, j], e, d, q) - ref.expanded_constant(zero[r, 0, j], e, d, q)) % q
                        assert added == (gad.lift(int(sel[r, b]), t) * (1 << (g * v)) % q if j == i else 0), (L, v, r, e, j)
                    touched[r, 0, i, e] = True
            assert np.array_equal(got[~touched], zero[~touched])  # nothing else changes: polynomial 1, the other primes, the other coefficients


# ---- the library without a device ----------------------------------------------------------------------------------------------
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
    assert "circular" in hdr.lower()  # he355_bfv_rgsw_encrypt_secret states its assumption


def test_refusals_are_decided_on_the_host(be, newlib):
    N, v = 4096, 20
    lib = newlib
    ctx = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    Lt = ctx.L
    E = ctx.bfv_gadget_count(Lt, v)[0]
    per = 2 * Lt * N
    a = np.full(4 * E * per + N, 0xABCD, dtype=np.uint64)      # selectors / slot ciphertexts, and room for an output behind them
    k = np.full(max(2 * E * per, 2 * 60 * 2 * N), 0xABCD, dtype=np.uint64)  # the key: 2 E rows at (Lt, v), 2 x 60 rows of 2 N words at (L, key_bits) = (1, 1)
    b = np.full(6 * E * per, 0xABCD, dtype=np.uint64)          # query ciphertexts / RGSW ciphertexts, and room for ciphertexts behind them
    pa, pk, pb = (x.ctypes.data_as(C.c_void_p) for x in (a, k, b))
    at = lambda base, words: C.c_void_p(base.value + 8 * words)
    se = lambda L=Lt, w=v, n=1, n_sel=2, first=3, count=64, sel=pa, dst=pb: lib.he355_bfv_selector_encrypt(ctx.h, L, w, n, n_sel, first, count, sel, 1, 0, dst)
    es = lambda L=Lt, w=v, dst=pb: lib.he355_bfv_rgsw_encrypt_secret(ctx.h, L, w, 1, 0, dst)
    fb = lambda L=Lt, w=v, kw=v, n=1, n_sel=2, ct=pa, sr=1, sk=1, key=pk, dst=pb: lib.he355_bfv_rgsw_from_bfv(ctx.h, L, w, kw, n, n_sel, ct, sr, sk, key, dst)
    bad = []
    for f in (se, es, fb):
        bad += [lambda f=f: f(L=0), lambda f=f: f(L=Lt + 1), lambda f=f: f(L=-1), lambda f=f: f(w=0), lambda f=f: f(w=64), lambda f=f: f(w=-1)]
    bad += [lambda: fb(kw=0), lambda: fb(kw=64), lambda: fb(kw=-1)]
    bad += [lambda: se(n_sel=0), lambda: fb(n_sel=0), lambda: se(n=0, n_sel=0), lambda: fb(n=0, n_sel=0),
            lambda: se(count=0), lambda: se(count=N + 1, n_sel=1), lambda: se(count=2 ** 63),
            lambda: se(first=64 - 2 * E + 1), lambda: se(n_sel=2 ** 62), lambda: se(first=2 ** 64 - 1), lambda: se(count=2 * E - 1, first=0),
            lambda: se(n=2 ** 31), lambda: fb(n=2 ** 31), lambda: fb(n_sel=2 ** 31), lambda: fb(n=2 ** 20, n_sel=2 ** 20),   # the grid
            lambda: fb(n=2, sr=2 ** 60), lambda: fb(sk=2 ** 60), lambda: fb(n=2, sr=2 ** 63),                               # strides that cannot be indices
            lambda: se(sel=pb), lambda: se(sel=at(pb, per - 1)), lambda: se(n=2, sel=at(pb, 2 * per - 1)),                  # the output on the selectors
            lambda: fb(ct=pb), lambda: fb(ct=at(pb, 4 * E * per - 1)), lambda: fb(dst=at(pa, 2 * E * per - 1)),             # ... on the ciphertexts
            lambda: fb(n_sel=1, sk=2, dst=at(pa, (2 * E - 2) * per)),                                                       # ... the last one at stride 2
            lambda: fb(key=pb), lambda: fb(key=at(pb, 4 * E * per - 1)), lambda: fb(dst=at(pk, 2 * E * per - 1))]           # ... on the key
    for i, f in enumerate(bad):
        assert f() == be.E_INVALID_ARGS, i
        assert len(lib.he355_last_error()) > 0, i
    # valid arguments: there is no device behind this context, and no CPU fallback
    for f in (se, lambda: se(L=1, w=63, n_sel=64, first=0), lambda: se(count=N, first=N - 2 * E), lambda: se(count=3 + 2 * E), lambda: se(n=0), es, lambda: es(L=1, w=1),
              fb, lambda: fb(L=1, w=63, kw=1), lambda: fb(n=0), lambda: fb(n_sel=1, sk=2, dst=at(pa, (2 * E - 1) * per)),
              lambda: se(sel=at(pb, per)), lambda: fb(ct=at(pb, 4 * E * per))):
        assert f() == be.E_DEVICE
        assert b"no CPU fallback" in lib.he355_last_error()
    ctx.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False)
    for f in (lambda: lib.he355_bfv_selector_encrypt(ck.h, 1, v, 1, 1, 0, 8, pa, 1, 0, pb), lambda: lib.he355_bfv_rgsw_encrypt_secret(ck.h, 1, v, 1, 0, pb),
              lambda: lib.he355_bfv_rgsw_from_bfv(ck.h, 1, v, v, 1, 1, pa, 1, 1, pk, pb)):
        assert f() == be.E_INVALID_ARGS
        assert b"BFV context" in lib.he355_last_error()
    ck.close()
    assert (a == 0xABCD).all() and (b == 0xABCD).all() and (k == 0xABCD).all()
