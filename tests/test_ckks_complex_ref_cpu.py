"""tests/ckks_complex_ref.py -- the definition the complex-slot calls are held to -- held to anchors the oracle already has, and the host
halves of the calls (he355_ckks_complex_unit, he355_ckks_complex_scalar_residues, he355_ckks_eval_poly_complex_plan: no device) held to it:

* the two facts the design rests on, at N = 1024, 2048 and 4096 on {60, 40, 40, 60}: NTT_{q_i}(J) is u_i where bit (log2 N - 2) of the index
  is 0 and q_i - u_i where it is 1; u_i^2 = -2 (mod q_i); J decodes to sqrt(2) i in every slot;
* the library's units and residue pairs equal the reference's (Python integers, v_im / math.sqrt(2.0));
* a combination equals, bit for bit, oracle.multiply_plain by NTT(A + B J) followed by add;
* the evaluator with zero imaginary parts equals the real reference; the complex plan equals the brute-force walk;
* accuracy with real keys at N = 2048, scale 2^40, slots in the unit disc: a degree-3 and a degree-7 complex polynomial p on the chains of
  tests/test_ckks_eval_poly_ref_cpu.py, decrypted, decoded and compared with numpy's p(x).  The bound is
  2 x (err(Re p) + err(Im p)): the errors of the REAL reference evaluator on the polynomials of the real and of the imaginary parts of the
  coefficients, on the same ciphertext in the same run; the factor 2 is for the second rounding (B) and J's sqrt(2) on the noise.
  Measured (profiles/ckks_complex.txt): the ratio err / (err(Re p) + err(Im p)) is 0.41 (degree 3), 0.59 (degree 7)
  and 0.54 (degree 7 on the five-prime chain).
No GPU."""
import importlib
import math
import os

import numpy as np
import pytest

import ckks_complex_ref as cref
import ckks_eval_poly_ref as ref
import oracle as ho
from test_ckks_eval_poly_ref_cpu import BITS5, BITS8, N, SCALE

CHAIN = [60, 40, 40, 60]
CUBIC = [0.5 + 0.1j, 0.15012 - 0.25j, 0.0, -0.0015930078125 + 0.05j]
SEPTIC = [0.1j, 0.31831 + 0.2j, 0.0, -0.10610 - 0.07j, 0.0, 0.06366j, 0.0, -0.04547 + 0.03j]
FACTOR = 2.0


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_the_two_facts_and_the_library_units(be, n):
    o = ho.Context(ho.SCHEME_CKKS, n, bit_sizes=CHAIN, sec128=False)
    g = be.Context(be.SCHEME_CKKS, n, bit_sizes=CHAIN, sec128=False)
    L, q = o.L, o.moduli
    u = cref.units(o, L)
    s = cref.half_of(n)
    assert s[0] == 0 and s[n // 4] == 1 and s[n // 2] == 0 and s[n // 4 - 1] == 0 and s[n - 1] == 1
    for i in range(L):
        J = o.ntt(i, cref.j_poly(n))
        assert np.array_equal(J, np.where(s == 0, np.uint64(u[i]), np.uint64(q[i] - u[i]))), i
        assert (u[i] * u[i] + 2) % q[i] == 0
    slots = ho.ckks_decode(o, np.stack([o.ntt(i, cref.j_poly(n)) for i in range(L)]), 1.0)
    assert np.max(np.abs(slots - math.sqrt(2.0) * 1j)) < 1e-14
    assert g.ckks_complex_unit(L) == u and g.ckks_complex_unit(1) == u[:1]
    for v in ((0.0, 0.0), (1.0, 0.0), (0.0, math.sqrt(2.0)), (-3.5, 2.5), (2.0 ** 40 * 0.3, -(2.0 ** 40) * 0.7), (2.0 ** 100, 2.0 ** 125), (0.49999, -0.70710678)):
        assert g.ckks_complex_scalar_residues(L, *v) == cref.scalar_residues(q, u, L, *v), v
        pair = cref.scalar_residues(q, u, L, *v)
        assert np.array_equal(cref.spread(pair, L, n), cref.scalar_plain(o, L, *v)), v  # the pair IS NTT(A + B J)
    assert g.ckks_complex_scalar_residues(L, 7.0, 0.0) == [g.ckks_scalar_residues(L, 7.0)] * 2
    for bad in ((float("inf"), 0.0), (0.0, float("nan")), (2.0 ** 126, 0.0), (0.0, 2.0 ** 127)):
        with pytest.raises(be.HE355Error) as ei:
            g.ckks_complex_scalar_residues(L, *bad)
        assert str(ei.value).count("he355_ckks_complex_scalar_residues: ")
    g.close()


@pytest.mark.parametrize("size", [2, 3])
def test_a_combination_is_multiply_plain_by_a_plus_bj_and_add(size):
    o = ho.Context(ho.SCHEME_CKKS, 1024, bit_sizes=[60, 40, 40, 40, 60], sec128=False)
    rng = np.random.default_rng(17 + size)
    L, q = 3, o.moduli
    u = cref.units(o, L)
    a, b = o.random_poly(rng, 3, size), o.random_poly(rng, 4, size)
    vals = [(2.0 ** 30 * 0.3, -(2.0 ** 30) * 0.9), (-5.0, 7.0), (2.0 ** 58, 2.0 ** 59)]
    terms = [a, b, a]
    pairs = [cref.scalar_residues(q, u, L, *v) for v in vals]
    cst = (123456.0, -654321.0)
    got = cref.combine(q, L, terms, pairs, cref.scalar_residues(q, u, L, *cst))
    acc = None
    for t, v in zip(terms, vals):
        td = t if t.shape[1] == L else o.mod_switch_drop(t, L)
        prod = o.multiply_plain(td, cref.scalar_plain(o, L, *v))
        acc = prod if acc is None else o.add(acc, prod)
    assert np.array_equal(cref.combine(q, L, terms, pairs), acc)
    assert np.array_equal(got, o.add_plain(acc, cref.scalar_plain(o, L, *cst)))
    assert np.array_equal(got, cref.combine_composed(o, L, terms, pairs, cref.scalar_residues(q, u, L, *cst)))
    edge = [[q[i] - 1 for i in range(L)], [q[i] - 1 for i in range(L)]]
    assert np.array_equal(cref.combine(q, L, [a], [edge]), ref.combine(q, L, [a], [edge[0]]))  # both halves equal: the real combination


@pytest.mark.parametrize("log_baby", [1, 2])
def test_zero_imaginary_parts_give_the_real_reference(log_baby):
    o = ho.Context(ho.SCHEME_CKKS, 1024, bit_sizes=[60, 40, 40, 40, 40, 60], sec128=False)
    rng = np.random.default_rng(5)
    rk = o.random_kswitch_key(rng)
    x = o.random_poly(rng, o.L, 2)
    for coeffs in ([0.25, -1.5], [0.5, 0.15012, 0.0, -0.0015930078125], [0.0, 0.3, 0.0, -0.1, 0.0, 0.06, 0.0, -0.04], [1.0, 0.0, 0.0, 0.0, 0.5]):
        want, ev = ref.eval_poly(o, x, coeffs, log_baby, SCALE, SCALE, rk, composed=True)
        got, cev = cref.eval_poly(o, x, [complex(c) for c in coeffs], log_baby, SCALE, SCALE, rk, composed=True)
        assert np.array_equal(got, want) and cev.counters() == ev.counters(), coeffs


SHAPES = {"cubic": CUBIC, "septic": SEPTIC, "imaginary line": [0.0, 1j], "1 + i x^4": [1.0, 0.0, 0.0, 0.0, 1j], "x + x^12": [0.0, 1.0 - 1j] + [0.0] * 10 + [2j],
          "dense 8": [0.3 + 0.01j * k for k in range(9)], "a tiny real part": [0.0, 1e-9 + 0.5j, 0.25]}


@pytest.mark.parametrize("log_baby", [1, 2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_complex_plan_against_the_brute_force_walk(be, name, log_baby):
    bits = [60] + [40] * 8 + [60]
    o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    coeffs, L = SHAPES[name], o.L
    ev = cref.Evaluator(o, coeffs, log_baby, L, SCALE, SCALE)
    ev.count()
    want = ev.counters()
    pl = g.ckks_eval_poly_complex_plan(L, coeffs, log_baby, SCALE, SCALE)
    assert {k: pl[k] for k in want} == want
    assert pl["powers_computed"] == ev.powers
    real_pl = g.ckks_eval_poly_plan(L, [1.0 if c != 0 else 0.0 for c in coeffs], log_baby, SCALE, SCALE)
    for k in ("depth", "L_out", "degree", "products", "combinations", "rescales", "drops", "adds", "powers", "powers_computed"):
        assert pl[k] == real_pl[k], k  # the tree is the real call's
    g.close()


def accuracy(bits, coeffs, seed):
    """(the complex tree's error, err(Re p), err(Im p)) on the same ciphertext of slots in the unit disc"""
    o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    rng = np.random.default_rng(seed)
    vals = np.sqrt(rng.uniform(0.0, 1.0, N // 2)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, N // 2))
    sk = o.keygen_secret(seed)
    pk, rk = o.keygen_public(sk, seed + 1), o.keygen_relin(sk, seed + 2)
    x = o.encrypt(pk, ho.ckks_encode(o, vals, SCALE), seed + 3)
    err = lambda ct, c: float(np.max(np.abs(ho.ckks_decode(o, o.decrypt_phase(ct, sk), SCALE) - np.polyval(c[::-1], vals))))
    re, im = [complex(c).real for c in coeffs], [complex(c).imag for c in coeffs]
    tree = err(cref.eval_poly(o, x, coeffs, 1, SCALE, SCALE, rk, composed=True)[0], [complex(c) for c in coeffs])
    return tree, err(ref.eval_poly(o, x, re, 1, SCALE, SCALE, rk, composed=True)[0], re), err(ref.eval_poly(o, x, im, 1, SCALE, SCALE, rk, composed=True)[0], im)


@pytest.mark.parametrize("name,bits,coeffs,seed", [("degree 3", BITS5, CUBIC, 300), ("degree 7", BITS8, SEPTIC, 400), ("degree 7, five primes", BITS5, SEPTIC, 400)])
def test_accuracy_of_a_complex_polynomial_against_the_real_reference(name, bits, coeffs, seed):
    tree, e_re, e_im = accuracy(bits, coeffs, seed)
    print(f"complex {name} on {bits}: tree {tree:.3e}  err(Re p) {e_re:.3e}  err(Im p) {e_im:.3e}  ratio {tree / (e_re + e_im):.2f}")
    assert e_re < 1e-6 and e_im < 1e-6  # (the reference route itself works)
    assert tree <= FACTOR * (e_re + e_im)
